"""The cases and yardsticks of the point prior (pba_set_point_prior): one extra residual block per point with a constant Jacobian and no
loss, in information form.  For point i with d = X_i - x0_i:  E_i = d^T Lambda_i d / 2, gradient Lambda_i d, Gauss-Newton block Lambda_i.

The yardsticks are lm_yardstick.Dense and lm_yardstick.PointBlocks with E added to the cost, Lambda d to the point gradient and Lambda
to H (or to the point blocks); they share nothing with the engine.  Windows: 96 x 128 images, K = (160, 160, 64, 48), as marginal_cases.

Priors (built from the window's START, never from a solve):
  depth   rank 1 along the optical axis of the point's reference camera (the slot of its first observation), Lambda = n n^T / sigma_z^2
          with n = R^T e_z, sigma_z = SIGMA_D z^2 / (BASELINE fx): what the drop-in class builds from a stereo disparity
  full    a full-rank SPD Lambda with mixed signs off the diagonal
  mixed   `depth` and `full` alternating, every third point with Lambda = 0 (no prior)
x0 is the start's point moved by a fixed pseudo-random offset of up to OFFSET of its depth, so E and its gradient are not zero at the start."""
import functools

import numpy as np

import anchors_cases
import lm_yardstick as lm
import marginal_cases
import wide_util
from photobundle_amd import se3

_IMG = dict(size=(96, 128), K=(160.0, 160.0, 64.0, 48.0))
EDGE_POINTS = (3, 63, 64, 65, 255, 256, 257)      # lane, wave and workgroup edges of the 256-lane point kernels
# The synthetic windows hold 8-bit intensities and points 10 to 40 units deep: a photometric point block V_i is of the order 1e5.  The
# depth factors are made as strong (baseline x fx / sigma_d = 1.6e5, depths of 20: Lambda of the order 1e5), so that a wrong addend shows
# in every compared quantity, and x0 sits close enough for E to stay a few per cent of the photometric cost.
SIGMA_D = 0.01       # disparity standard deviation [pixels]
BASELINE = 10.0      # stereo baseline [world units]
OFFSET = 0.002
KINDS = ("depth", "full", "mixed")
GAUGE = "gauge-3-dense-64-points-anchor-0"

# name: (window, constant slots).  window: make_window arguments, "causal" (the 5 x 60 causal Huber window of anchors_cases),
# ("boundary", slots) = anchors_cases.boundary_window, ("wide", slots) = that window banded by wide_util.shape_window
CASES = {"3-dense-%d-points-anchor-0" % n: (dict(n_frames=3, n_points=n, radius=1, **_IMG), (0,)) for n in EDGE_POINTS}
CASES["5x60-causal-huber-anchors-0-4"] = ("causal", (0, 4))
CASES["16-slots-anchor-0"] = (("boundary", 16), (0,))                  # 15 free cameras: the narrow limit
CASES["20-slots-anchors-0-1"] = (("wide", 20), (0, 1))                 # more than 16 slots: a wide window by its shape
CASES[GAUGE] = (dict(n_frames=3, n_points=64, radius=1, seed_offset=0, **_IMG), (0,))
WIDE = "20-slots-anchors-0-1"
CAUSAL = "5x60-causal-huber-anchors-0-4"
# the cases of the first-step and trace comparisons (the gauge case has tests of its own)
STEP_CASES = sorted(k for k in CASES if k != GAUGE)
TRACE_CASES = ("3-dense-65-points-anchor-0", CAUSAL, "16-slots-anchor-0", WIDE)
REF_ITERATIONS = 12
BOUNDARY_ITERATIONS = 5      # the loss-free causal windows of 16 and more slots: test_gpu_marginal.py's note on rejected candidates


@functools.lru_cache(maxsize=None)
def window(name):
    """The problem of a case (shared, never modified)."""
    from photobundle_amd import synthetic
    w = CASES[name][0]
    if w == "causal":
        return anchors_cases.trace_case(marginal_cases.CAUSAL)[0]
    if isinstance(w, tuple) and w[0] == "boundary":
        return anchors_cases.boundary_window(w[1])
    if isinstance(w, tuple):
        p = wide_util.shape_window(anchors_cases.boundary_window(w[1]), band=9)
        assert p.n_frames > 16 and len(np.unique(p.obs_slot)) == p.n_frames
        return p
    return synthetic.make_window(**w)


def anchors_of(name):
    return tuple(CASES[name][1])


# ---- the priors ----------------------------------------------------------------------------------------------------------------------------
def sym3(L6):
    """[n, 6] upper triangles row by row (00 01 02 11 12 22) -> [n, 3, 3]."""
    L6 = np.asarray(L6, np.float64)
    L = np.zeros((len(L6), 3, 3))
    for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        L[:, i, j] = L[:, j, i] = L6[:, k]
    return L


def tri6(L):
    L = np.asarray(L, np.float64)
    return np.ascontiguousarray(np.stack([L[:, 0, 0], L[:, 0, 1], L[:, 0, 2], L[:, 1, 1], L[:, 1, 2], L[:, 2, 2]], axis=1))


def ref_slots(p):
    """The slot of every point's first observation (the lists are sorted by point, then by slot)."""
    first = np.searchsorted(np.asarray(p.obs_point), np.arange(p.n_points))
    return np.asarray(p.obs_slot)[first]


def depth_prior(p, cams=None, xyz=None, sigma=SIGMA_D, baseline=BASELINE):
    """Lambda [n, 3, 3] = n n^T / sigma_z^2 along the reference camera's optical axis, at the depth the point has there."""
    cams = p.cams if cams is None else cams
    xyz = p.xyz if xyz is None else xyz
    fx = float(p.K[0])
    L = np.zeros((p.n_points, 3, 3))
    for i, s in enumerate(ref_slots(p)):
        R, t = se3.angle_axis_to_matrix(cams[s][:3]), np.asarray(cams[s][3:6])
        z = float((R @ xyz[i] + t)[2])
        n = R.T @ np.array([0.0, 0.0, 1.0])
        sz = sigma * z * z / (baseline * fx)
        L[i] = np.outer(n, n) / (sz * sz)
    return L


def full_prior(p, seed=7):
    """Full-rank SPD blocks with mixed signs off the diagonal, of the size of the depth factors."""
    rng = np.random.RandomState(seed)
    scale = np.array([np.trace(b) for b in depth_prior(p)])
    L = np.zeros((p.n_points, 3, 3))
    for i in range(p.n_points):
        A = rng.uniform(-1.0, 1.0, (3, 3))
        B = A @ A.T + 0.25 * np.eye(3)
        B[0, 1] = B[1, 0] = -abs(B[0, 1])
        B[0, 2] = B[2, 0] = abs(B[0, 2])
        B[1, 2] = B[2, 1] = -abs(B[1, 2])
        assert np.linalg.eigvalsh(B).min() > 0
        L[i] = B * (scale[i] / np.trace(B))
    return L


@functools.lru_cache(maxsize=None)
def prior(name, kind):
    """(x0 [n, 3], Lambda6 [n, 6]) of a case, float64 and contiguous: what pba_set_point_prior takes (shared, never modified)."""
    return prior_of(window(name), kind)


def prior_of(p, kind):
    """... of any window."""
    rng = np.random.RandomState(11)
    depth = np.linalg.norm(p.xyz, axis=1)
    x0 = np.ascontiguousarray(p.xyz + rng.uniform(-1.0, 1.0, p.xyz.shape) * (OFFSET * depth)[:, None])
    if kind == "depth":
        L = depth_prior(p)
    elif kind == "full":
        L = full_prior(p)
    else:
        assert kind == "mixed"
        L = np.where((np.arange(p.n_points) % 2 == 0)[:, None, None], depth_prior(p), full_prior(p))
        L[2::3] = 0.0
        assert p.n_points < 3 or (np.abs(L).reshape(p.n_points, -1).max(1) == 0).any()
    L6 = tri6(L)
    assert np.array_equal(sym3(L6), L)
    return x0, L6


def energy(x0, L6, xyz, dtype=np.float64):
    """E_pts = sum_i d^T Lambda_i d / 2 at the points xyz."""
    d = np.asarray(xyz, dtype) - np.asarray(x0, dtype)
    return float(0.5 * np.einsum("ni,nij,nj->", d, np.asarray(sym3(L6), dtype), d))


def gathered(x0, L6, point_map):
    """The rows of the points that survive a cull (pba_cull's point_map: new index or -1), in their new order."""
    keep = np.asarray(point_map) >= 0
    assert np.array_equal(np.asarray(point_map)[keep], np.arange(int(keep.sum())))
    return np.ascontiguousarray(x0[keep]), np.ascontiguousarray(L6[keep])


# ---- the yardsticks ------------------------------------------------------------------------------------------------------------------------
class DenseWithPointPrior(lm.Dense):
    """lm_yardstick.Dense plus one residual block per point with a constant Jacobian and no loss: E joins the cost (last, after the
    photometric sum), Lambda_i d the gradient of the point's columns, Lambda_i its diagonal block of H."""

    def __init__(self, p, slots, x0, L6, **kw):
        super().__init__(p, slots, **kw)
        assert self.rays is None
        self.x0, self.L6, self.L = np.asarray(x0, np.float64), np.asarray(L6, np.float64), sym3(L6)

    def prior_cost(self, state):
        return energy(self.x0, self.L6, state[1])

    def cost(self, state):
        return super().cost(state) + self.prior_cost(state)

    def linearize(self, state):
        lin = super().linearize(state)                              # (its cost is self.cost: E is in)
        H, g, nc = lin["H"], lin["gradient"], self.n_cam
        d = state[1] - self.x0
        g[nc:] += np.einsum("nij,nj->ni", self.L, d).ravel()
        for i in range(self.p.n_points):
            H[nc + 3 * i:nc + 3 * i + 3, nc + 3 * i:nc + 3 * i + 3] += self.L[i]
        return dict(lin, gradient=g, diagonal=np.diag(H).copy(), H=H)


class PointBlocksWithPrior(lm.PointBlocks):
    """lm_yardstick.PointBlocks with the same addends: the cameras-constant mode."""

    def __init__(self, p, x0, L6, **kw):
        super().__init__(p, **kw)
        assert self.rays is None
        self.x0, self.L6, self.L = np.asarray(x0, np.float64), np.asarray(L6, np.float64), sym3(L6)

    def prior_cost(self, x):
        return energy(self.x0, self.L6, x)

    def _evaluate(self, x, blocks):
        cost, V, g = super()._evaluate(x, blocks)
        g = g + np.einsum("nij,nj->ni", self.L, x - self.x0)
        if V is not None:
            V = V + self.L
        return cost + self.prior_cost(x), V, g


@functools.lru_cache(maxsize=None)
def yardstick(name, kind, mode="full"):
    """(the yardstick's solve over REF_ITERATIONS, the number of compared iterations) of a case, shared."""
    p = window(name)
    x0, L6 = prior(name, kind)
    prog = DenseWithPointPrior(p, anchors_of(name), x0, L6) if mode == "full" else PointBlocksWithPrior(p, x0, L6)
    res = prog.solve(max_num_iterations=REF_ITERATIONS)
    return res, lm.compared_iterations(res)


def reduced_unit_diagonal(H, n_cam):
    """The unit-diagonal reduced camera matrix of a dense H (float64 Schur elimination of the point columns; a singular point block
    raises LinAlgError)."""
    S = H[:n_cam, :n_cam] - H[:n_cam, n_cam:] @ np.linalg.solve(H[n_cam:, n_cam:], H[n_cam:, :n_cam])
    d = 1.0 / np.sqrt(np.diag(S))
    return S * d[:, None] * d[None, :]
