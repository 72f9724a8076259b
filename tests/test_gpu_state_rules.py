"""-m gpu: what the engine derives from its inputs is dropped when an input changes (invalidate() in photobundle_amd/csrc/pba_engine.hip).
Pattern of every case: an engine fills every cache of its mode (linearize, step, accept, linearize, step), ONE input is changed, then
linearize + step run again -- and must give the bits of a fresh engine built straight into the final inputs and the same mode: the
cost, the step's 32-double scalar block (pba_internal_step) and the reduced system (the per-point blocks in the cameras-constant mode).
A cache that outlives its input shows as different bits.  Shapes are small, stale state shows at any size: 3 frames x 40 points, radius 1,
on a 120 x 160 image; the wide window has 17 frames x 60 points (one slot more than the narrow tables hold).

The frame cases (a frame upload is an input like the others) do not hold before the invalidation table: pba_set_frame_* dropped
nothing, so linearize returned the cost of the records sampled from the old image.

One thing is not a cache and still depends on the engine's history: the derivative matrices dR of a camera's geometry.  pba_set_cameras
computes them in k_cam_geom (cam_geom_one), an accepted step of the narrow full mode in the reduced solve (cam_geom_finish, pba_solve.h),
and the two differ in the last bit (the compiler contracts the two chains differently).  The sampler does not read dR, the Schur
elimination does: with the accepted cameras left as the solve wrote them, the warmed engine and a fresh one agree in the cost and in
every record, and differ by 1e-16 in the reduced system (entries up to 0.66) and by 2e-14 relative in the point part of the model cost
change -- on the commit before the table and after it alike, and with any event that does not go through pba_set_cameras.  The full
mode therefore hands the accepted cameras back through pba_set_cameras right after pba_accept, as a caller does that keeps the window on
the host; both cache fills around it stay.  The pose-only mode, the wide window and the cameras-constant modes need no such step (their
geometry is cam_geom_one's, or never moves) and run the plain sequence.

The trust-region radius is 1e-2: at the solver's initial 1e4 the first inverse-depth step of these windows leaves the domain (rho <= 0)."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from photobundle_amd import _lib, synthetic
from photobundle_amd.engine import Engine, default_solver_options

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(radius=1, size=(120, 160), K=(200.0, 200.0, 80.0, 60.0))
RADIUS = 1e-2


def _num_scal():
    """kNumScal of csrc/pba_lm_rules.h: doubles of a step's scalar block."""
    src = open(os.path.join(ROOT, "photobundle_amd", "csrc", "pba_lm_rules.h")).read()
    return int(re.search(r"kNumScal\s*=\s*(\d+)", src).group(1))


@dataclasses.dataclass
class Inputs:
    """Everything a caller hands the engine, and the mode it asks for."""
    images: np.ndarray
    xyz: np.ndarray
    cams: np.ndarray
    constant_slots: tuple
    points_const: bool = False
    cams_const: bool = False
    rays: np.ndarray = None         # inverse depth: set_inverse_depth(rays, rho) after set_problem
    rho: np.ndarray = None
    hand_back_cameras: bool = False      # warmed(): pba_set_cameras with the accepted cameras right after pba_accept (module docstring)


@pytest.fixture(scope="module")
def windows():
    narrow = synthetic.make_window(n_frames=3, n_points=40, **SMALL)
    wide = synthetic.make_window(n_frames=17, n_points=60, visibility="causal", **SMALL)
    assert len(np.unique(wide.obs_slot)) == 17
    return dict(narrow=narrow, wide=wide)


MODES = {
    "full": dict(hand_back_cameras=True),
    "points_const": dict(points_const=True),
    "cams_const": dict(cams_const=True),
    "inverse_depth_cams_const": dict(cams_const=True, inverse_depth=True),
    "wide": dict(window="wide"),
}


def start_inputs(windows, mode):
    kw = dict(MODES[mode])
    p = windows[kw.pop("window", "narrow")]
    rays, rho = synthetic.inverse_depth_rays(p) if kw.pop("inverse_depth", False) else (None, None)
    return p, Inputs(images=p.images, xyz=p.xyz, cams=p.cams, constant_slots=(0,), rays=rays, rho=rho, **kw)


def set_problem_and_mode(e, p, inp):
    """set_problem switches inverse depth and both constant modes off: the caller asks for them again."""
    e.set_problem(inp.xyz, p.desc, p.obs_point, p.obs_slot, p.weights)
    if inp.rays is not None:
        e.set_inverse_depth(inp.rays, inp.rho)
    if inp.points_const:
        e.set_points_constant()
    if inp.cams_const:
        e.set_cameras_constant()


def build(p, inp):
    rows, cols = inp.images.shape[1:]
    e = Engine(rows, cols, p.K, p.radius, p.n_frames, huber=p.huber, keep_reduced_system=True)
    for s, im in enumerate(inp.images):
        e.set_frame(s, im)
    set_problem_and_mode(e, p, inp)
    e.set_cameras(inp.cams, constant_slots=inp.constant_slots)
    return e


def raw_step(e, init_scale):
    """pba_step with the raw scalar block: (step info fields, kNumScal doubles)."""
    o, info, scal = default_solver_options(), _lib.StepInfo(), np.zeros(_num_scal())
    rc = _lib.lib().pba_internal_step(e._h, C.c_double(RADIUS), C.c_int32(int(init_scale)), C.byref(o), C.byref(info),
                                      scal.ctypes.data_as(C.c_void_p), C.c_int(0))
    e._check(rc, "pba_internal_step")
    return info, scal


def measure(e, inp):
    """(cost, scalar block, system matrix, right-hand side) of linearize + one step with fresh Jacobi scales."""
    cost = e.linearize()
    info, scal = raw_step(e, True)
    assert info.linear_solver_ok and info.eval_ok and np.isfinite(scal).all()
    return (cost, scal) + (e.point_system() if inp.cams_const else e.reduced_system())


def assert_same_bits(got, want):
    assert got[0].hex() == want[0].hex(), "cost"
    slots = [k for k in range(len(want[1])) if got[1][k].tobytes() != want[1][k].tobytes()]
    assert not slots, "scalar block, slots %s: %s against %s" % (slots, [got[1][k].hex() for k in slots], [want[1][k].hex() for k in slots])
    assert got[2].tobytes() == want[2].tobytes(), "system matrix: largest difference %.3e" % np.abs(got[2] - want[2]).max()
    assert got[3].tobytes() == want[3].tobytes(), "right-hand side: largest difference %.3e" % np.abs(got[3] - want[3]).max()


def warmed(p, inp):
    """An engine with every cache of its mode filled, two steps into the problem, and its inputs as they stand then."""
    e = build(p, inp)
    e.linearize()
    raw_step(e, True)
    e.accept()
    if inp.hand_back_cameras:
        e.set_cameras(e.get_state()[0], constant_slots=inp.constant_slots)
    e.linearize()
    raw_step(e, False)
    cams, x = e.get_state()
    now = dataclasses.replace(inp, cams=cams)
    return e, (dataclasses.replace(now, rho=x[:, 0].copy()) if inp.rays is not None else dataclasses.replace(now, xyz=x))


def _noise(shape, scale, seed):
    return scale * np.random.default_rng(seed).standard_normal(shape)


# ---- the events: each changes one input of the warmed engine and returns the inputs as they stand afterwards --------------------------
def ev_cameras(e, p, now):
    fin = dataclasses.replace(now, cams=now.cams + _noise(now.cams.shape, 1e-3, 1))
    e.set_cameras(fin.cams, constant_slots=fin.constant_slots)
    return fin


def ev_anchor_mask(e, p, now):
    fin = dataclasses.replace(now, constant_slots=(0, p.n_frames - 1))
    e.set_cameras(fin.cams, constant_slots=fin.constant_slots)
    return fin


def ev_inverse_depth(e, p, now):
    if now.rays is None:
        rays, rho = synthetic.inverse_depth_rays(p)
    else:
        rays, rho = now.rays, now.rho * (1.0 + _noise(now.rho.shape, 1e-3, 2))
    fin = dataclasses.replace(now, rays=rays, rho=rho)
    e.set_inverse_depth(rays, rho)
    return fin


def ev_toggle_points_const(e, p, now):
    e.set_points_constant(not now.points_const)
    e.set_points_constant(now.points_const)
    return now


def ev_toggle_cams_const(e, p, now):
    e.set_cameras_constant(not now.cams_const)
    e.set_cameras_constant(now.cams_const)
    return now


def ev_problem(e, p, now):
    if now.rays is None:
        fin = dataclasses.replace(now, xyz=now.xyz + _noise(now.xyz.shape, 1e-3, 3))
    else:
        fin = dataclasses.replace(now, rho=now.rho * (1.0 + _noise(now.rho.shape, 1e-3, 3)))
    set_problem_and_mode(e, p, fin)
    return fin


# (mode, event): a wide window refuses inverse depth, and each constant mode refuses the other being switched on
CASES = [(m, ev) for m in MODES for ev in (ev_cameras, ev_anchor_mask, ev_problem)]
CASES += [(m, ev_inverse_depth) for m in MODES if m != "wide"]
CASES += [(m, ev_toggle_points_const) for m in ("full", "points_const", "wide")]
CASES += [(m, ev_toggle_cams_const) for m in ("full", "cams_const", "inverse_depth_cams_const", "wide")]


@pytest.mark.parametrize("mode,event", CASES, ids=["%s-%s" % (m, ev.__name__[3:]) for m, ev in CASES])
def test_a_setter_after_cached_state_equals_a_fresh_engine(windows, mode, event):
    p, inp = start_inputs(windows, mode)
    e, now = warmed(p, inp)
    with e:
        fin = event(e, p, now)
        got = measure(e, fin)
    with build(p, fin) as fresh:
        want = measure(fresh, fin)
    print("%s / %s: cost %.17g (fresh engine %.17g)" % (mode, event.__name__[3:], got[0], want[0]))
    assert_same_bits(got, want)


@pytest.mark.parametrize("mode", ["full", "points_const", "cams_const"])
def test_a_frame_upload_after_cached_state_equals_a_fresh_engine(windows, mode):
    p, inp = start_inputs(windows, mode)
    e, now = warmed(p, inp)
    slot = 1
    assert slot in p.obs_slot
    images = now.images.copy()
    images[slot] = now.images[slot][::-1, ::-1]
    fin = dataclasses.replace(now, images=images)
    with e:
        before = e.linearize()
        e.set_frame(slot, images[slot])
        got = measure(e, fin)
    with build(p, fin) as fresh:
        want = measure(fresh, fin)
    print("%s / frame: cost before the upload %.17g, after %.17g (fresh engine %.17g)" % (mode, before, got[0], want[0]))
    assert_same_bits(got, want)
    assert got[0] != before
