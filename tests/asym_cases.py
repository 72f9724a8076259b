"""Inputs that no symmetry hides: patch weights that differ from every rotation and flip of themselves, and a calibration with
fx != fy and cx != cy.  The windows of tests/test_asymmetric_inputs_cpu.py (their conditions) and tests/test_gpu_asymmetric_inputs.py (the
engine on them), and the yardstick runs the two files share.

Every window elsewhere in the suite has unit or Gaussian weights (unchanged by the eight symmetries of the square) and fx == fy, so a
weight read at the transposed or mirrored tap, or a swapped pair of focal lengths, changes nothing those tests can see."""
import copy
import functools

import numpy as np

import lm_yardstick as lm

SIZE = (120, 160)
ANISO_K = (230.0, 170.0, 83.0, 57.0)          # fx / fy = 1.35, cx != cy
_IMG = dict(size=SIZE, K=ANISO_K)
# The class tests of tests/test_gpu_dropin_class.py: ANISO_K for the 120 x 160 sequence; for the 160 x 224 pyramid sequence ANISO_K x 1.4
# with the principal point rounded to the pixel.  (At exactly x 1.4, cx = 116.2 and cy = 79.8, the second coarse window -- 65 points, 34
# iterations -- is not determinate in double precision: the oracle's own extended-precision run leaves its double run at the third
# iteration, ends 8e-7 away in cost and 3e-7 in the cameras, and the finer windows that start from that pose amplify it to 5e-3.  One
# sample position rounds to the neighbouring float, the event gpu_util.referee_parity describes.  test_asymmetric_inputs_cpu.py asserts
# for both sequences that every window is determinate.)
PYRAMID_SIZE = (160, 224)
PYRAMID_K = (322.0, 238.0, 116.0, 80.0)
WEIGHT_SEED = 20261021
D4_MIN_DISTANCE = 0.25
REF_ITERATIONS = 6                             # iteration limit of the yardstick's traces


def d4_images(w):
    """The seven non-identity images of a square patch [W, W] under the symmetries of the square, by name."""
    return {"rot90": np.rot90(w, 1), "rot180": np.rot90(w, 2), "rot270": np.rot90(w, 3), "flip-rows": w[::-1, :], "flip-columns": w[:, ::-1],
            "transpose": w.T, "anti-transpose": np.rot90(w, 2).T}


@functools.lru_cache(maxsize=None)
def _weights(radius):
    W = 2 * radius + 1
    w = np.random.default_rng(WEIGHT_SEED + radius).uniform(0.25, 1.75, size=(W, W))
    # an exact 0 on an edge tap next to a corner and an exact 1 in the opposite corner: no symmetry of the square maps one onto the other
    w[0, 1], w[W - 1, W - 1] = 0.0, 1.0
    for name, img in d4_images(w).items():
        assert np.abs(w - img).max() >= D4_MIN_DISTANCE, (radius, name, np.abs(w - img).max())
    assert (w != 1.0).any()                      # the engine takes its unit-weight kernels when every weight is exactly 1
    assert (w == 0.0).sum() == 1 and (w == 1.0).sum() == 1
    w = np.ascontiguousarray(w.reshape(-1))
    w.setflags(write=False)
    return w


def asymmetric_weights(radius):
    """(2 radius + 1)^2 weights, row-major: uniform in [0.25, 1.75], one exactly 0 and one exactly 1, at least D4_MIN_DISTANCE away
    from each of their seven rotated / flipped images."""
    return _weights(radius).copy()


def d4_weights(radius):
    """{name: flat weights} of the seven non-identity images of asymmetric_weights(radius)."""
    W = 2 * radius + 1
    return {k: np.ascontiguousarray(v).reshape(-1) for k, v in d4_images(asymmetric_weights(radius).reshape(W, W)).items()}


def asym(p):
    """A copy of window p with the asymmetric weights of its radius (p itself, often a shared cached window, stays as it is)."""
    q = copy.copy(p)
    q.weights = asymmetric_weights(p.radius)
    return q


def swapped_focal(p):
    """A copy of p with fx and fy exchanged (the sensitivity condition of the reference)."""
    q = copy.copy(p)
    fx, fy, cx, cy = p.K
    q.K = (fy, fx, cx, cy)
    return q


WINDOWS = {
    "A4": dict(n_frames=4, n_points=60, radius=2, seed_offset=21),
    "A3h": dict(n_frames=3, n_points=40, radius=1, huber=0.05, seed_offset=21),
    "A5": dict(n_frames=5, n_points=60, radius=1, huber=0.05, visibility="causal", seed_offset=21),
    "A17": dict(n_frames=17, n_points=60, radius=1, visibility="causal", seed_offset=21),
    "A4c3": dict(n_frames=4, n_points=60, radius=1, seed_offset=21, channels="IntensityAndGradient"),
    "R4": dict(n_frames=3, n_points=40, radius=4, seed_offset=21),
    "R5": dict(n_frames=3, n_points=40, radius=5, seed_offset=21),
    # The inverse-depth traces.  From make_window's default start the FIRST step of A4 sends a far point (the wall at 40 m, rho = 0.025)
    # below zero, in the full mode and in the structure-only mode alike: behind the ray origin, outside the parameterisation's domain,
    # where the oracle returns some finite cost and the device's sampler a failed evaluation (anchors_cases.py and points_only_cases.py
    # met the same).  So on A4 the inverse-depth modes are compared through their system and first step, and their traces run on these
    # two: the gentle start of the scipy comparisons, the structure-only one with its cameras at the ground truth as in
    # points_only_cases.py.  Of seeds 0..11 and 21, seed 11 is the one whose full-mode candidates all stay positive (smallest 0.0037
    # against a smallest initial 0.025); seed 21 keeps the structure-only ones at 0.022 and above.  test_asymmetric_inputs_cpu.py asserts
    # the domain.
    "G11": dict(n_frames=4, n_points=60, radius=2, rot_deg=0.05, trans=0.01, depth_noise=0.005, seed_offset=11),
    "G21gt": dict(n_frames=4, n_points=60, radius=2, rot_deg=0.05, trans=0.01, depth_noise=0.005, seed_offset=21, cameras="ground-truth"),
}


@functools.lru_cache(maxsize=None)
def window(name):
    """The window of a name (shared, never modified): 120 x 160 images, ANISO_K, asymmetric weights."""
    from photobundle_amd import synthetic
    kw = dict(WINDOWS[name])
    kind, cameras = kw.pop("channels", None), kw.pop("cameras", None)
    if kind is not None:
        kw["channel_fn"] = synthetic.channel_fn(kind)
    p = asym(synthetic.make_window(**kw, **_IMG))
    if cameras == "ground-truth":
        p.cams = np.array(p.meta["cams_gt"], dtype=np.float64)
    return p


def border_problem(radius, channels):
    """The problem of tests/test_gpu_border_sweep.py (patch footprints on, inside and outside every image limit) with asymmetric weights."""
    import test_gpu_border_sweep as sweep
    p = sweep._problem(radius, channels, seed=10 * radius + channels)
    p.weights = asymmetric_weights(radius)
    return p


# ---- the programs of the GPU cases and their yardstick runs, computed once and shared ---------------------------------------------------
# name: (window, constant slots, parameterisation)
DENSE_CASES = {
    "A4-anchors-0-3": ("A4", (0, 3), "world"),
    "A5-anchors-0-4": ("A5", (0, 4), "world"),
    "A17-anchor-0": ("A17", (0,), "world"),                     # 16 free cameras: the wide chain
    "A4-inverse-depth-anchors-0-3": ("A4", (0, 3), "inverse-depth"),          # system and first step only
    "G11-inverse-depth-anchors-0-3": ("G11", (0, 3), "inverse-depth"),
    # the drivers: one constant slot, as pba_set_cameras gives it
    "A4-anchor-0": ("A4", (0,), "world"),
    "A3h-anchor-0": ("A3h", (0,), "world"),
    "R4-anchor-0": ("R4", (0,), "world"),
    "R5-anchor-0": ("R5", (0,), "world"),
}
POSE_CASES = ("A3h", "A5")
STRUCTURE_CASES = {"A4-world": ("A4", "world"), "A4-inverse-depth": ("A4", "inverse-depth"), "G21gt-inverse-depth": ("G21gt", "inverse-depth")}
FIRST_STEP_ONLY = ("A4-inverse-depth-anchors-0-3", "A4-inverse-depth")      # no trace: see WINDOWS
COVARIANCE_CASE = ("A4", (0, 3))
MARGINAL_CASES = {"A4-anchor-0-drop-0": ("A4", (0,), (0,)), "A4-anchor-0-drop-1": ("A4", (0,), (1,))}
PRIOR_SOLVE = "A4-anchor-0-drop-1"             # the marginalisation whose prior one solve is run with
CULL_CASE = ("A5", (0,), 3)                    # window, constant slots, iterations before the costs are read
ADMIT_CASE = ("A4", (0,), 3)
ADMIT_MARGIN_PX, ADMIT_MARGIN_DEPTH = 1.0, 0.1  # the yardstick's margins at ITS state after the iterations; the engine's: 1e-6 px


@functools.lru_cache(maxsize=None)
def rays_of(name):
    from photobundle_amd import synthetic
    return synthetic.inverse_depth_rays(window(name))


def dense_program(case):
    name, slots, param = DENSE_CASES[case]
    p = window(name)
    rays, rho = rays_of(name) if param == "inverse-depth" else (None, None)
    return p, slots, rays, rho, lm.Dense(p, slots, rays, rho)


@functools.lru_cache(maxsize=None)
def dense_first_step(case):
    return dense_program(case)[4].first_step(radius=1e4)


@functools.lru_cache(maxsize=None)
def dense_trace(case):
    """(result, compared iterations) of the yardstick's solve of a Dense case."""
    res = dense_program(case)[4].solve(max_num_iterations=REF_ITERATIONS)
    return res, lm.compared_iterations(res)


def pose_program(name):
    return lm.CameraBlocks(window(name))


@functools.lru_cache(maxsize=None)
def pose_trace(name):
    res = pose_program(name).solve(max_num_iterations=REF_ITERATIONS)
    return res, lm.compared_iterations(res)


def structure_program(case):
    name, param = STRUCTURE_CASES[case]
    p = window(name)
    rays, rho = rays_of(name) if param == "inverse-depth" else (None, None)
    return p, rays, rho, lm.PointBlocks(p, rays, rho)


@functools.lru_cache(maxsize=None)
def structure_trace(case):
    res = structure_program(case)[3].solve(max_num_iterations=REF_ITERATIONS)
    return res, lm.compared_iterations(res)


@functools.lru_cache(maxsize=None)
def marginal_reference(case):
    import marginal_cases as mc
    name, anchors, drop = MARGINAL_CASES[case]
    return mc.reference(window(name), anchors, drop)


@functools.lru_cache(maxsize=None)
def prior_trace():
    """(result, compared iterations, prior) of the prior-augmented yardstick on the window the prior came from.  (A4 is dense: every
    point is seen by the dropped slot, so the window without the marginalised points is empty; the prior is an extra block on the whole
    window, which exercises the same kernels.)"""
    import marginal_cases as mc
    name, anchors, _ = MARGINAL_CASES[PRIOR_SOLVE]
    prior = mc.as_prior(marginal_reference(PRIOR_SOLVE))
    res = mc.DenseWithPrior(window(name), anchors, prior).solve(max_num_iterations=REF_ITERATIONS)
    return res, lm.compared_iterations(res), prior


def decisions(res, n_cmp):
    """(accepted, rejected) valid steps among the compared iterations of a yardstick trace."""
    its = res["iterations"][1:n_cmp]
    return (sum(1 for i in its if i["step_is_valid"] and i["step_is_successful"]),
            sum(1 for i in its if i["step_is_valid"] and not i["step_is_successful"]))
