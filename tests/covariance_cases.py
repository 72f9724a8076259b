"""The cases and the reference of the covariance output (pba_covariance), 96 x 128 images.

Reference: H = J^T J of the reduced program from lm_yardstick.Dense(...).linearize(state)["H"] (the block sums of oracle.block_products in
the two constant modes), inverted by the extended-precision (numpy longdouble) Cholesky below.  Errors are measured in correlation
units, |dSigma_ij| / sqrt(Sigma_ii Sigma_jj); the bar of a case is 10 x kappa x 1e-12, kappa the 2-norm condition number of the
unit-diagonal H: 1e-12 is the project's record-parity bar, an inverse amplifies it by the condition number, and the factor 10 covers a
structured rather than random difference and another summation order.  Every case must have kappa <= 1e8 and a reference camera pivot
>= 1e-5 (test_covariance_cpu.py asserts it; a seed that breaks it is replaced, not waived)."""
import functools

import numpy as np

import anchors_cases
import lm_yardstick as lm
from oracle import oracle

LD = np.longdouble
RECORD_BAR = 1e-12
KAPPA_MAX = 1e8
PIVOT_MIN = 1e-5

_IMG = dict(size=(96, 128), K=(160.0, 160.0, 64.0, 48.0))

# name: (window, constant slots).  window: a trace case of anchors_cases, ("boundary", slots in the window) or make_window arguments
FULL_CASES = {
    "3x40-dense-r1-anchors-0-2": ("trace", (0, 2)),
    "5x60-causal-huber-anchors-0-4": ("trace", (0, 4)),
    "5x60-causal-huber-anchors-0-1-2": ("trace", (0, 1, 2)),
    "4x50-dense-r2-anchors-1-3": ("trace", (1, 3)),
    "16-slots-anchors-0-1": (("boundary", 16), (0, 1)),
    "17-slots-anchors-0-1": (("boundary", 17), (0, 1)),
    "17-slots-anchors-0-16": (("boundary", 17), (0, 16)),
    "17-slots-16-anchors": (("boundary", 17), tuple(range(16))),
    "20-slots-12-anchors": (("boundary", 20), tuple(range(12))),
    "32-slots-anchors-0-31": (("boundary", 32), (0, 31)),
}
TRACE_NAMES = [k for k, v in FULL_CASES.items() if v[0] == "trace"]
EDGE_POINTS = (1, 63, 64, 65, 255, 256, 257)       # lane, wave and workgroup edges of the one-lane-per-point kernels
# (one point gives a free camera two independent equations per observation: 9 unknowns, rank <= 6.  That window is singular by counting,
# no seed qualifies it, so in the full mode it runs under the rank-deficiency rule; the structure-only mode compares it like the others.
# Two points leave 12 unknowns against at most 12 equations and are singular too; THREE points are the smallest window whose camera is
# determined, and that window stands in for the small-grid edge of the full mode: one workgroup with three busy lanes)
SMALLEST_FULL = 3
for _n in (SMALLEST_FULL,) + EDGE_POINTS[1:]:
    FULL_CASES["3-dense-%d-points-anchors-0-2" % _n] = (dict(n_frames=3, n_points=_n, radius=1, **_IMG), (0, 2))
# the gauge-open variants: one constant slot
ONE_ANCHOR = {
    "3x40-dense-r1-anchor-0": ("3x40-dense-r1-anchors-0-2", (0,)),
    "5x60-causal-huber-anchor-0": ("5x60-causal-huber-anchors-0-4", (0,)),
    "17-slots-anchor-0": ("17-slots-anchors-0-1", (0,)),
    "32-slots-anchor-0": ("32-slots-anchors-0-31", (0,)),
}
ONE_POINT = dict(n_frames=3, n_points=1, radius=1, **_IMG)
INVERSE_DEPTH = "4x60-dense-r1-inverse-depth-anchors-0-3"


@functools.lru_cache(maxsize=None)
def window(name):
    """The problem of a case (shared, never modified)."""
    from photobundle_amd import synthetic
    if name in ONE_ANCHOR:
        return window(ONE_ANCHOR[name][0])
    if name == INVERSE_DEPTH:
        return anchors_cases.trace_case(name)[0]
    w = FULL_CASES[name][0]
    if w == "trace":
        return anchors_cases.trace_case(name)[0]
    if isinstance(w, tuple):
        return anchors_cases.boundary_window(w[1])
    return synthetic.make_window(**w)


def slots_of(name):
    return tuple((ONE_ANCHOR.get(name) or FULL_CASES[name])[1])


# ---- extended-precision algebra ----------------------------------------------------------------------------------------------------------
def unit_diagonal(A):
    """(D^-1/2 A D^-1/2, D^-1/2) with D = diag A, in the precision of A."""
    d = 1 / np.sqrt(np.diag(A))
    return A * d[:, None] * d[None, :], d


def cholesky_pivots(A):
    """Right-looking Cholesky of A in its own precision.  Returns (L, pivots): pivots[j] is the diagonal entry the root is taken of; the
    factorisation stops at the first pivot that is not positive (L is then None and the pivots end with the offender)."""
    A = np.array(A, copy=True)
    n = len(A)
    piv = []
    for j in range(n):
        d = A[j, j]
        piv.append(d)
        if not (d > 0 and np.isfinite(d)):
            return None, np.array(piv)
        A[j:, j] /= np.sqrt(d)
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return np.tril(A), np.array(piv)


def inverse_ld(A):
    """(A^-1 as float64, smallest pivot of the unit-diagonal A) through the longdouble Cholesky of the unit-diagonal matrix."""
    Au, d = unit_diagonal(np.asarray(A, LD))
    L, piv = cholesky_pivots(Au)
    if L is None:
        raise np.linalg.LinAlgError("pivot %r at column %d" % (float(piv[-1]), len(piv) - 1))
    n = len(Au)
    X = np.zeros((n, n), LD)                      # L^-1, row by row
    for i in range(n):
        X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
        X[i, i] = 1 / L[i, i]
    inv = (X.T @ X) * d[:, None] * d[None, :]
    return np.asarray(inv, np.float64), float(piv.min())


def min_pivot(A, dtype=LD):
    """Smallest pivot of the unit-diagonal A; the first non-positive one when the factorisation fails."""
    _, piv = cholesky_pivots(unit_diagonal(np.asarray(A, dtype))[0])
    return float(piv[-1]) if not (piv[-1] > 0) else float(piv.min())


def correlation_error(got, ref):
    """max |got - ref|_ij / sqrt(ref_ii ref_jj) over a matrix, or over a stack of blocks [k, d, d]."""
    got, ref = np.asarray(got), np.asarray(ref)
    if ref.size == 0:
        return 0.0
    s = np.sqrt(np.einsum("...ii->...i", ref))
    return float(np.max(np.abs(got - ref) / (s[..., :, None] * s[..., None, :])))


def kappa(H):
    return float(np.linalg.cond(unit_diagonal(np.asarray(H, np.float64))[0]))


# ---- references ------------------------------------------------------------------------------------------------------------------------
def full_reference(p, slots, state=None):
    """The full mode at `state` = (cams, xyz) (default: the start).  dict(H, n_cam, cam_cov, point_cov [n, 3, 3], kappa, bar,
    min_cam_pivot, min_point_pivot, cost), everything from the dense H by the longdouble inverse."""
    prog = lm.Dense(p, slots)
    lin = prog.linearize(prog.start() if state is None else state)
    H, nc = lin["H"], prog.n_cam
    inv, _ = inverse_ld(H)
    n_pts = p.n_points
    pts = np.stack([inv[nc + 3 * i:nc + 3 * i + 3, nc + 3 * i:nc + 3 * i + 3] for i in range(n_pts)])
    Hl = np.asarray(H, LD)
    V = [Hl[nc + 3 * i:nc + 3 * i + 3, nc + 3 * i:nc + 3 * i + 3] for i in range(n_pts)]
    S = Hl[:nc, :nc].copy()
    for i in range(n_pts):
        W = Hl[:nc, nc + 3 * i:nc + 3 * i + 3]
        S -= W @ np.asarray(inverse_ld(V[i])[0], LD) @ W.T
    k = kappa(H)
    return dict(H=H, n_cam=nc, cam_cov=inv[:nc, :nc], point_cov=pts, kappa=k, bar=10 * k * RECORD_BAR, min_cam_pivot=min_pivot(S),
                min_point_pivot=min(min_pivot(v) for v in V), cost=lin["cost"])


def block_sums(p, slots, cams=None, xyz=None):
    """(free slots, U [k, 6, 6], W {(free index, point): [6, 3]}, V [n, 3, 3]) summed from oracle.block_products in list order."""
    free = lm.free_slots(p, slots)
    col = {c: i for i, c in enumerate(free)}
    bp = oracle.block_products(p, cams=p.cams if cams is None else cams, xyz=p.xyz if xyz is None else xyz)
    U, V, W = np.zeros((len(free), 6, 6)), np.zeros((p.n_points, 3, 3)), {}
    for o in range(p.n_obs):
        i, c = int(p.obs_point[o]), int(p.obs_slot[o])
        V[i] += bp["JpJp"][o]
        if c in col:
            U[col[c]] += bp["JcJc"][o]
            W[(col[c], i)] = W.get((col[c], i), 0) + bp["JcJp"][o]
    return free, U, W, V


def schur_covariance(free, U, W, V, dtype=np.float64):
    """The three block formulas of include/pba.h in `dtype`: (Sigma_cc, Sigma_pp [n, 3, 3], S)."""
    nc, n_pts = 6 * len(free), len(V)
    inv = (lambda a: np.asarray(inverse_ld(a)[0], LD)) if dtype is LD else np.linalg.inv
    P = [inv(np.asarray(v, dtype)) for v in V]
    S = np.zeros((nc, nc), dtype)
    for a in range(len(free)):
        S[6 * a:6 * a + 6, 6 * a:6 * a + 6] = U[a]
    by_point = {}
    for (a, i), w in W.items():
        by_point.setdefault(i, []).append((a, np.asarray(w, dtype)))
    for i, lst in by_point.items():
        for a, wa in lst:
            for b, wb in lst:
                S[6 * a:6 * a + 6, 6 * b:6 * b + 6] -= wa @ P[i] @ wb.T
    Scc = inv(S)
    Spp = np.zeros((n_pts, 3, 3), dtype)
    for i in range(n_pts):
        Spp[i] = P[i]
        for a, wa in by_point.get(i, []):
            for b, wb in by_point.get(i, []):
                Spp[i] += (P[i] @ wa.T) @ Scc[6 * a:6 * a + 6, 6 * b:6 * b + 6] @ (wb @ P[i])
    return np.asarray(Scc, np.float64), np.asarray(Spp, np.float64), S


def pose_reference(p, slots, cams=None):
    """Pose-only mode: (program slots, blockdiag(U_a^-1) dense, U [k, 6, 6], program cost)."""
    prog = lm.CameraBlocks(p, slots)
    lin = prog.linearize(np.array(p.cams if cams is None else cams, np.float64))
    n = 6 * len(prog.cols)
    cov = np.zeros((n, n))
    for k, u in enumerate(lin["U"]):
        cov[6 * k:6 * k + 6, 6 * k:6 * k + 6] = inverse_ld(u)[0]
    return prog.cols, cov, lin["U"], lin["cost"]


def structure_reference(p, rays=None, rho=None, x=None):
    """Structure-only mode: (V^-1 [n, d, d], V [n, d, d], cost), d = 1 with inverse depths."""
    prog = lm.PointBlocks(p, rays, rho)
    lin = prog.linearize(prog.start() if x is None else x)
    return np.stack([inverse_ld(v)[0] for v in lin["V"]]), lin["V"], lin["cost"]
