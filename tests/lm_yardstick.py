"""The yardstick of every constant-block mode and of the oracle's solver options: ONE numpy Levenberg-Marquardt loop, written from Ceres'
documented rules (TrustRegionMinimizer + LevenbergMarquardtStrategy), that drives a small program object:

  scaling        1 / (1 + sqrt(diag J^T J)) per column, fixed at iteration 0 (ones with jacobi_scaling off)
  damping        clip(diag of the scaled J^T J, min_lm_diagonal, max_lm_diagonal) / radius
  step           the program's exact solve of its damped normal equations, model cost change -m^T (r + m / 2)
  invalid step   a failed linear solve or a model cost change <= 0: radius / 2, / 4, ... as for a rejected step, and the solve fails once
                 max_num_consecutive_invalid_steps of them follow each other
  decision       relative decrease > min_relative_decrease; radius / max(1/3, 1 - (2 rho - 1)^3) on success, / 2, / 4, ... on failure; a
                 rejected step logs the candidate's cost
  termination    gradient tolerance after a successful step; parameter and function tolerance on the candidate (the solve ends without
                 logging that iteration); iteration limit; minimum radius

The loop knows nothing about cameras or points.  A program answers start() (the initial state), linearize(x) (a dict with cost,
gradient, diagonal and, where blocks leave the program, fixed_cost), cost(x), step(lin, scale, radius, min_diag, max_diag) (a dict with
delta, model_cost_change, linear_solver_ok), apply(x, delta), x_norm(x), points(x) (the point parameters, or None) and
num_residual_blocks.  The four programs keep their own evaluators and their own algebra:

  CameraBlocks      pose-only (pba_set_points_constant): the free cameras that have a residual block, one 6 x 6 block each; the blocks
                    of the constant cameras leave the program, their loss-corrected cost is fixed_cost (in initial_cost / final_cost, not
                    in the iterations)
  PointBlocks       structure-only (pba_set_cameras_constant): one 3 x 3 block per point (1 x 1 with inverse depths); a block that is
                    not positive definite fails the whole step
  Dense             anchor frames (pba_set_cameras_anchored): the cameras outside a set of slots and all points, Cholesky of the full
                    dense normal equations; first_step() also returns the reduced camera system by explicit Schur elimination
  ExplicitJacobian  the full problem with one constant slot from an explicit Jacobian, H = Js^T Js + D^2

With inverse depths the parameter of point i is rho_i on the fixed world ray (o_i, d_i), X_i = o_i + d_i / rho_i, and the oracle's
world-point pieces go through the chain rule dX / drho = -d / rho^2.  Evaluations come from the unchanged oracle (linearize,
block_products, cost, eval_block).  Shares no code with the engine or with the oracle's own solver."""
import numpy as np

from oracle import oracle

DEFAULTS = dict(max_num_iterations=500, function_tolerance=1e-6, gradient_tolerance=1e-6, parameter_tolerance=1e-6,
                initial_trust_region_radius=1e4, max_trust_region_radius=1e16, min_trust_region_radius=1e-32,
                min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32, max_num_consecutive_invalid_steps=5,
                jacobi_scaling=True)


def options_of(o):
    """The loop's options read off an options object of the oracle."""
    return {k: getattr(o, k) for k in DEFAULTS}


def block_costs(p, sq):
    a = p.huber
    rho = np.where((a > 0) & (sq > a * a), 2 * a * np.sqrt(sq) - a * a, sq)
    return 0.5 * rho


def huber_cost(p, cams, xyz):
    return float(np.sum(block_costs(p, oracle.linearize(p, cams=cams, xyz=xyz, blocks=False)["block_sqnorm"])))


def initial_points(p, rays=None, rho=None):
    """The point parameters [n_points, d]: world points (d = 3), or inverse depths (d = 1)."""
    return np.array(p.xyz, np.float64) if rays is None else np.array(rho, np.float64).reshape(-1, 1)


def world_points(x, rays=None):
    return x if rays is None else rays[:, :3] + rays[:, 3:] / x


def _dx_drho(x, rays):
    return -rays[:, 3:] / (x * x)


def free_slots(p, slots):
    """The camera columns: slots outside the constant set, ascending."""
    slots = {int(s) for s in slots}
    assert all(0 <= s < p.n_frames for s in slots)
    return [c for c in range(p.n_frames) if c not in slots]


def dense_system(p, cams=None, xyz=None):
    """Dense corrected Jacobian + residual from per-block oracle evaluations (free columns only, one constant slot)."""
    P = p.patch_len
    cols_c = {c: 6 * i for i, c in enumerate([c for c in range(p.n_frames) if c != p.fixed_slot])}
    n_cam = 6 * len(cols_c)
    J = np.zeros((p.n_obs * P, n_cam + 3 * p.n_points))
    r = np.zeros(p.n_obs * P)
    for o in range(p.n_obs):
        rb, jc, jp = oracle.eval_block(p, o, cams=cams, xyz=xyz)
        s = rb @ rb
        k = np.sqrt(p.huber / np.sqrt(s)) if p.huber > 0 and s > p.huber ** 2 else 1.0
        rows = slice(o * P, (o + 1) * P)
        r[rows] = k * rb
        c = p.obs_slot[o]
        if c in cols_c:
            J[rows, cols_c[c]:cols_c[c] + 6] = k * jc
        q = n_cam + 3 * p.obs_point[o]
        J[rows, q:q + 3] = k * jp
    return J, r, n_cam


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


# ---- the loop --------------------------------------------------------------------------------------------------------------------------
def _copy(x):
    return tuple(a.copy() for a in x) if isinstance(x, tuple) else x.copy()


def _min_point(prog, x):
    pts = prog.points(x)
    return None if pts is None else float(pts.min())


def solve(prog, **options):
    """Runs the loop on a program.  Returns dict(iterations=[dict], states=[the state after every logged iteration], x (the final
    state), initial_cost, final_cost, fixed_cost, num_residual_blocks, message, min_candidate (smallest point parameter of any evaluated
    candidate: inverse depths must stay positive))."""
    o = dict(DEFAULTS)
    for k in options:
        if k not in o:
            raise KeyError(k)
    o.update(options)
    x = prog.start()
    lin = prog.linearize(x)
    cost, g, fixed_cost = lin["cost"], lin["gradient"], lin.get("fixed_cost", 0.0)
    scale = 1.0 / (1.0 + np.sqrt(lin["diagonal"])) if o["jacobi_scaling"] else np.ones_like(lin["diagonal"])
    radius, dec = o["initial_trust_region_radius"], 2.0
    its = [dict(iteration=0, step_is_valid=1, step_is_successful=1, cost=cost, cost_change=0.0, gradient_max_norm=float(np.abs(g).max()),
                gradient_norm=float(np.linalg.norm(g)), step_norm=0.0, relative_decrease=0.0, trust_region_radius=radius,
                model_cost_change=0.0)]
    states = [_copy(x)]
    minimum_cost, invalid, message = cost, 0, None
    min_candidate = _min_point(prog, x)
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
        st = prog.step(lin, scale, radius, o["min_lm_diagonal"], o["max_lm_diagonal"])
        it["model_cost_change"] = st["model_cost_change"]
        if not (st["linear_solver_ok"] and st["model_cost_change"] > 0.0):
            invalid += 1
            if invalid >= o["max_num_consecutive_invalid_steps"]:
                message = "Number of consecutive invalid steps more than max_num_consecutive_invalid_steps."
                its.append(it); states.append(_copy(x))
                break
            radius /= dec
            dec *= 2.0
            it["trust_region_radius"] = radius
            its.append(it); states.append(_copy(x))
            continue
        invalid = 0
        it["step_is_valid"] = 1
        cand = prog.apply(x, st["delta"])
        it["step_norm"] = float(np.linalg.norm(st["delta"]))
        if it["step_norm"] <= o["parameter_tolerance"] * (prog.x_norm(x) + o["parameter_tolerance"]):
            message = "Parameter tolerance reached."
            break
        if min_candidate is not None:
            it["min_candidate"] = _min_point(prog, cand)
            min_candidate = min(min_candidate, it["min_candidate"])
        cand_cost = prog.cost(cand)
        it["cost_change"] = cost - cand_cost
        if abs(it["cost_change"]) <= o["function_tolerance"] * cost:
            message = "Function tolerance reached."
            break
        rd = it["cost_change"] / st["model_cost_change"]
        it["relative_decrease"] = rd
        if rd > o["min_relative_decrease"]:
            x = cand
            lin = prog.linearize(x)
            cost, g = lin["cost"], lin["gradient"]
            radius = min(o["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - (2.0 * rd - 1.0) ** 3))
            dec = 2.0
            it.update(step_is_successful=1, cost=cost, gradient_max_norm=float(np.abs(g).max()), gradient_norm=float(np.linalg.norm(g)))
            minimum_cost = min(minimum_cost, cost)
        else:
            radius /= dec
            dec *= 2.0
            it["cost"] = cand_cost       # Ceres >= 1.12 logs the candidate's cost for a rejected step
        it["trust_region_radius"] = radius
        its.append(it); states.append(_copy(x))
    return dict(iterations=its, states=states, x=x, initial_cost=its[0]["cost"] + fixed_cost, final_cost=minimum_cost + fixed_cost,
                fixed_cost=fixed_cost, num_residual_blocks=prog.num_residual_blocks, message=message, min_candidate=min_candidate)


def _first_step(prog, radius, min_diag, max_diag):
    """The first LM step of a program: what step() returns, plus scale, gradient (unscaled), cost, fixed_cost, x_norm, step_norm and
    num_residual_blocks."""
    x = prog.start()
    lin = prog.linearize(x)
    scale = 1.0 / (1.0 + np.sqrt(lin["diagonal"]))
    st = prog.step(lin, scale, radius, min_diag, max_diag)
    return dict(st, scale=scale, gradient=lin["gradient"], cost=lin["cost"], fixed_cost=lin.get("fixed_cost", 0.0), x_norm=prog.x_norm(x),
                step_norm=float(np.linalg.norm(st["delta"])), num_residual_blocks=prog.num_residual_blocks)


def _block_system(B, g, scale, radius, min_diag, max_diag):
    """Scaled blocks, scaled gradient and the scaled + damped blocks of a block-diagonal program."""
    Bs = B * scale[:, :, None] * scale[:, None, :]
    D2 = np.clip(np.einsum("kii->ki", Bs), min_diag, max_diag) / radius
    return Bs, g * scale, Bs + np.einsum("ki,ij->kij", D2, np.eye(g.shape[1]))


def _block_result(S, Bs, gs, y, scale, ok):
    # -m^T (r + m / 2) with m = J step, step = -y:  y^T gs - y^T Bs y / 2
    mcc = float(np.sum(y * gs) - 0.5 * np.einsum("ki,kij,kj->", y, Bs, y))
    return dict(S=S, rhs=gs, delta=-y * scale, model_cost_change=mcc, linear_solver_ok=ok)


# ---- the four programs -----------------------------------------------------------------------------------------------------------------
class CameraBlocks:
    """Camera columns only, the points as they are (or `xyz`).  slots: the constant slots, by default p.fixed_slot when that is >= 0."""

    def __init__(self, p, slots=None, xyz=None):
        if slots is None:
            slots = (p.fixed_slot,) if p.fixed_slot >= 0 else ()
        self.p, self.xyz = p, p.xyz if xyz is None else xyz
        self.slots = sorted({int(s) for s in slots})
        # the reduced program: free cameras with at least one residual block, and the blocks that are not a constant camera's
        self.cols = [int(c) for c in np.unique(np.asarray(p.obs_slot)) if c not in self.slots]
        self.in_program = ~np.isin(np.asarray(p.obs_slot), self.slots)
        self.num_residual_blocks = int(self.in_program.sum())

    def start(self):
        return np.array(self.p.cams, dtype=np.float64)

    def _evaluate(self, cams, blocks):
        lin = oracle.linearize(self.p, cams=cams, xyz=self.xyz, blocks=blocks)
        c = block_costs(self.p, lin["block_sqnorm"])
        fixed = 0.0
        for a in self.slots:       # the constant cameras' blocks, summed in ascending slot order
            fixed += float(c[np.asarray(self.p.obs_slot) == a].sum())
        return lin, float(c[self.in_program].sum()), fixed

    def linearize(self, cams):
        lin, cost, fixed = self._evaluate(cams, True)
        U = lin["U"][self.cols]
        return dict(cost=cost, fixed_cost=fixed, gradient=lin["grad_cams"][self.cols], diagonal=np.einsum("kii->ki", U), U=U)

    def cost(self, cams):
        return self._evaluate(cams, False)[1]

    def step(self, lin, scale, radius, min_diag, max_diag):
        Us, gs, S = _block_system(lin["U"], lin["gradient"], scale, radius, min_diag, max_diag)
        ok = True
        y = np.zeros_like(gs)
        for k in range(len(S)):
            try:
                L = np.linalg.cholesky(S[k])
                y[k] = np.linalg.solve(L.T, np.linalg.solve(L, gs[k]))
            except np.linalg.LinAlgError:
                ok = False
        ok = ok and bool(np.all(np.isfinite(y)))
        return _block_result(S, Us, gs, y, scale, ok)

    def apply(self, cams, delta):
        cand = cams.copy()
        cand[self.cols] += delta
        return cand

    def x_norm(self, cams):
        return float(np.linalg.norm(cams[self.cols]))

    def points(self, cams):
        return None

    def first_step(self, radius=1e4, min_diag=1e-6, max_diag=1e32):
        """dict(cols (program slots), scale, S [k, 6, 6] (scaled + damped blocks), rhs [k, 6], delta [k, 6], model_cost_change,
        gradient [k, 6], cost, fixed_cost, ...)."""
        return dict(_first_step(self, radius, min_diag, max_diag), cols=self.cols)

    def solve(self, **options):
        """The loop's result with the final cameras as `cams`."""
        if not self.cols:
            raise ValueError("empty program: no free camera has a residual block")
        res = solve(self, **options)
        return dict(res, cams=res["x"])


class PointBlocks:
    """Point columns only, the cameras as they are; every residual block depends on a point, so none leaves the program."""

    def __init__(self, p, rays=None, rho=None, autodiff=True):
        self.p, self.rays, self.rho, self.autodiff = p, rays, rho, autodiff
        self.num_residual_blocks = int(p.n_obs)

    def start(self):
        return initial_points(self.p, self.rays, self.rho)

    def _evaluate(self, x, blocks):
        lin = oracle.linearize(self.p, autodiff=self.autodiff, cams=self.p.cams, xyz=world_points(x, self.rays), blocks=blocks)
        cost = float(block_costs(self.p, lin["block_sqnorm"]).sum())
        V, g = lin.get("V"), lin["grad_pts"]
        if self.rays is not None:
            q = _dx_drho(x, self.rays)
            g = np.einsum("ni,ni->n", q, g)[:, None]
            if V is not None:
                V = np.einsum("ni,nij,nj->n", q, V, q)[:, None, None]
        return cost, V, g

    def linearize(self, x):
        cost, V, g = self._evaluate(x, True)
        return dict(cost=cost, gradient=g, diagonal=np.einsum("kii->ki", V), V=V)

    def cost(self, x):
        return self._evaluate(x, False)[0]

    def step(self, lin, scale, radius, min_diag, max_diag):
        Vs, gs, S = _block_system(lin["V"], lin["gradient"], scale, radius, min_diag, max_diag)
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
        return _block_result(S, Vs, gs, y, scale, ok)

    def apply(self, x, delta):
        return x + delta

    def x_norm(self, x):
        return float(np.linalg.norm(x))

    def points(self, x):
        return x

    def first_step(self, radius=1e4, min_diag=1e-6, max_diag=1e32):
        """dict(x, scale, S [n, d, d] (scaled + damped blocks), rhs [n, d], delta [n, d], model_cost_change, gradient [n, d], cost,
        linear_solver_ok, ...)."""
        return dict(_first_step(self, radius, min_diag, max_diag), x=self.start())

    def solve(self, **options):
        """The loop's result with the final parameters as `x` and their world points as `xyz`."""
        res = solve(self, **options)
        return dict(res, xyz=world_points(res["x"], self.rays), inverse_depth=self.rays is not None)


def _apply_dense(free, n_cam, state, delta):
    cams, x = state
    cand_c = cams.copy()
    for i, c in enumerate(free):
        cand_c[c] += delta[6 * i:6 * i + 6]
    return cand_c, x + delta[n_cam:].reshape(x.shape)


class Dense:
    """The cameras outside `slots` (ascending, 6 columns each) and then d columns per point; the state is (cams, point parameters).
    Every residual block stays (each depends on a free point); a constant camera's blocks still feed the point blocks and the point
    gradient."""

    def __init__(self, p, slots, rays=None, rho=None, autodiff=True):
        self.p, self.rays, self.rho, self.autodiff = p, rays, rho, autodiff
        self.free = free_slots(p, slots)
        used = set(int(s) for s in np.unique(np.asarray(p.obs_slot)))
        self.live = [c for c in self.free if c in used]       # the camera parameter blocks of the Ceres program
        self.n_cam = 6 * len(self.free)
        self.num_residual_blocks = int(p.n_obs)

    def start(self):
        return np.array(self.p.cams, np.float64), initial_points(self.p, self.rays, self.rho)

    def cost(self, state):
        _, sq = oracle.cost(self.p, cams=state[0], xyz=world_points(state[1], self.rays))
        return float(block_costs(self.p, sq).sum())

    def linearize(self, state):
        """H = J^T J and gradient = J^T r from oracle.block_products."""
        p, (cams, x), n_cam = self.p, state, self.n_cam
        col = {c: 6 * i for i, c in enumerate(self.free)}
        d = x.shape[1]
        bp = oracle.block_products(p, autodiff=self.autodiff, cams=cams, xyz=world_points(x, self.rays))
        JcJp, JpJp, Jpr = bp["JcJp"], bp["JpJp"], bp["Jpr"]
        if self.rays is not None:
            q = _dx_drho(x, self.rays)[np.asarray(p.obs_point)]           # dX / drho of every block's point
            JcJp = np.einsum("oij,oj->oi", JcJp, q)[:, :, None]
            JpJp = np.einsum("oi,oij,oj->o", q, JpJp, q)[:, None, None]
            Jpr = np.einsum("oi,oi->o", q, Jpr)[:, None]
        N = n_cam + d * p.n_points
        H, g = np.zeros((N, N)), np.zeros(N)
        for o in range(p.n_obs):
            pc = n_cam + d * int(p.obs_point[o])
            H[pc:pc + d, pc:pc + d] += JpJp[o]
            g[pc:pc + d] += Jpr[o]
            c = int(p.obs_slot[o])
            if c in col:
                cc = col[c]
                H[cc:cc + 6, cc:cc + 6] += bp["JcJc"][o]
                g[cc:cc + 6] += bp["Jcr"][o]
                H[cc:cc + 6, pc:pc + d] += JcJp[o]
                H[pc:pc + d, cc:cc + 6] += JcJp[o].T
        return dict(cost=self.cost(state), gradient=g, diagonal=np.diag(H), H=H)

    def step(self, lin, scale, radius, min_diag, max_diag):
        Hs = lin["H"] * scale[:, None] * scale[None, :]
        gs = lin["gradient"] * scale
        D2 = np.clip(np.diag(Hs), min_diag, max_diag) / radius
        A = Hs + np.diag(D2)
        try:
            L = np.linalg.cholesky(A)
            y = np.linalg.solve(L.T, np.linalg.solve(L, gs))
            ok = bool(np.all(np.isfinite(y)))
        except np.linalg.LinAlgError:
            y, ok = np.zeros_like(gs), False
        # -m^T (r + m / 2) with m = J step, step = -y:  y^T gs - y^T Hs y / 2
        mcc = float(y @ gs - 0.5 * y @ Hs @ y)
        return dict(A=A, gs=gs, delta=-y * scale, model_cost_change=mcc, linear_solver_ok=ok)

    def apply(self, state, delta):
        return _apply_dense(self.free, self.n_cam, state, delta)

    def x_norm(self, state):
        return float(np.sqrt((state[0][self.live] ** 2).sum() + (state[1] ** 2).sum()))

    def points(self, state):
        return state[1]

    def first_step(self, radius=1e4, min_diag=1e-6, max_diag=1e32):
        """dict(free, n_cam, scale, S [n_cam, n_cam] and rhs [n_cam] (the scaled + damped reduced camera system, by explicit Schur
        elimination of the point columns of the dense matrix), delta_c [n_free, 6], delta_p [n_points, d], model_cost_change, gradient
        (unscaled), cost, x_norm, step_norm, linear_solver_ok, ...)."""
        st, n_cam = _first_step(self, radius, min_diag, max_diag), self.n_cam
        A, gs = st["A"], st["gs"]
        App_inv_Apc = np.linalg.solve(A[n_cam:, n_cam:], A[n_cam:, :n_cam])
        S = A[:n_cam, :n_cam] - A[:n_cam, n_cam:] @ App_inv_Apc
        rhs = gs[:n_cam] - App_inv_Apc.T @ gs[n_cam:]
        return dict(st, free=self.free, n_cam=n_cam, S=S, rhs=rhs, delta_c=st["delta"][:n_cam].reshape(-1, 6),
                    delta_p=st["delta"][n_cam:].reshape(self.p.n_points, -1))

    def solve(self, **options):
        """The loop's result with the final state as `cams` and `x`, and the world points as `xyz`."""
        res = solve(self, **options)
        cams, x = res["x"]
        return dict(res, cams=cams, x=x, xyz=world_points(x, self.rays), inverse_depth=self.rays is not None)


class ExplicitJacobian:
    """The full problem with p.fixed_slot constant, from the explicit corrected Jacobian of dense_system(); the state is (cams, xyz)."""

    def __init__(self, p):
        self.p = p
        self.free = [c for c in range(p.n_frames) if c != p.fixed_slot]
        self.n_cam = 6 * len(self.free)
        self.num_residual_blocks = int(p.n_obs)

    def start(self):
        return self.p.cams.copy(), self.p.xyz.copy()

    def cost(self, state):
        return huber_cost(self.p, *state)

    def linearize(self, state):
        J, r, _ = dense_system(self.p, *state)
        return dict(cost=self.cost(state), gradient=J.T @ r, diagonal=(J * J).sum(0), J=J, r=r)

    def step(self, lin, scale, radius, min_diag, max_diag):
        Js, r = lin["J"] * scale, lin["r"]
        D2 = np.clip((Js * Js).sum(0), min_diag, max_diag) / radius
        H = Js.T @ Js + np.diag(D2)
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            return dict(H=H, delta=np.zeros(len(scale)), model_cost_change=0.0, linear_solver_ok=False)
        step = -np.linalg.solve(L.T, np.linalg.solve(L, Js.T @ r))
        model = Js @ step
        return dict(H=H, delta=step * scale, model_cost_change=-model @ (r + model / 2), linear_solver_ok=True)

    def apply(self, state, delta):
        return _apply_dense(self.free, self.n_cam, state, delta)

    def x_norm(self, state):
        return np.sqrt(sum((state[0][c] ** 2).sum() for c in self.free) + (state[1] ** 2).sum())

    def points(self, state):
        return state[1]

    def first_step(self, radius=1e4, min_diag=1e-6, max_diag=1e32):
        """dict(H (scaled + damped), scale, delta, model_cost_change, gradient (unscaled), cost, x_norm, step_norm, ...)."""
        return _first_step(self, radius, min_diag, max_diag)

    def solve(self, **options):
        """The loop's result with the final state as `cams` and `xyz`."""
        res = solve(self, **options)
        return dict(res, cams=res["x"][0], xyz=res["x"][1])
