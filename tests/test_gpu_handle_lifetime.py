"""-m gpu: lifetimes of the three handles (pba_engine, pba_stereo, pba_sgm) now that one registry owns their device and pinned memory
(photobundle_amd/csrc/pba_alloc.h, pba_handle.h).  Every case compares result BITS: a buffer that is released too early, kept at a stale
capacity or handed to the wrong owner shows as different cameras, points or iteration records, or as a failing call.  Shapes are the
smoke run's: 120 x 160, 4 frames, radius 2.  Device-wide free memory is not asserted (on a shared card that figure belongs to every job
on it); the poisoned path keeps its test in tests/test_gpu_resident.py."""
import numpy as np
import pytest

from photobundle_amd import stereo, synthetic
from photobundle_amd.engine import Engine, default_solver_options

pytestmark = pytest.mark.gpu

SIZE, K, FRAMES, RADIUS = (120, 160), (200.0, 200.0, 80.0, 60.0), 4, 2


def window(n_points):
    return synthetic.make_window(n_frames=FRAMES, n_points=n_points, radius=RADIUS, size=SIZE, K=K)


def engine(p):
    return Engine(SIZE[0], SIZE[1], p.K, p.radius, p.n_frames, huber=p.huber, device=0)


def bits(res):
    """Everything a solve returns but its clocks: cameras, points, and every iteration record field by field."""
    its = tuple(tuple((k, v.hex() if isinstance(v, float) else v) for k, v in sorted(it.items()) if "time" not in k) for it in res["iterations"])
    return res["cams"].tobytes(), res["xyz"].tobytes(), its, res["termination_type"]


def solve(e, p, iterations):
    e.load(p)
    return bits(e.solve(default_solver_options(max_num_iterations=iterations)))


def test_grow_and_shrink_equal_fresh_engines():
    """One engine sees windows of 100, 700 and 100 points: buffers are kept, regrown, then kept larger than needed."""
    windows = [window(n) for n in (100, 700, 100)]
    with engine(windows[0]) as e:
        reused = [solve(e, p, 3) for p in windows]
    for p, got in zip(windows, reused):
        with engine(p) as fresh:
            want = solve(fresh, p, 3)
        assert len(want[2]) >= 2
        assert got == want, p.n_points


def test_create_solve_destroy_cycles():
    """25 times: an engine, a block matcher and a semi-global matcher are created, used once and destroyed; the last cycle returns the
    first one's bits."""
    p = window(300)
    rng = np.random.default_rng(7)
    left = rng.integers(0, 256, (48, 96), dtype=np.uint8)
    right = np.roll(left, -5, axis=1)
    first = None
    for cycle in range(25):
        with engine(p) as e:
            out = [solve(e, p, 2)]
            with stereo.StereoBM(48, 96, number_of_disparities=16, sad_window_size=9) as bm:
                out += [a.tobytes() for a in bm.compute(left, right, bf=100.0)]
            with stereo.StereoSGM(48, 96, number_of_disparities=16) as sgm:
                out += [a.tobytes() for a in sgm.compute_all(left, right, bf=100.0)]
        if first is None:
            first = out
    assert len(out[0][2]) >= 2 and len(out) == 6
    assert out == first


def test_first_use_buffers_are_released_with_the_engine():
    """The buffers of the pose-only and structure-only modes and of the device time stamps appear on first use, after create: an engine
    that has grown all of them is destroyed, and a fresh one repeats the first solve."""
    p = window(300)
    with engine(p) as e:
        want = solve(e, p, 3)
        e.set_points_constant()
        e.linearize()
        assert e.step(1e4, init_scale=True)["linear_solver_ok"]
        e.set_points_constant(False)
        e.set_cameras_constant()
        e.linearize()
        assert e.step(1e4, init_scale=True)["linear_solver_ok"]
        e.set_cameras_constant(False)
        e.set_profiling(2)
        assert len(e.solve(default_solver_options(max_num_iterations=3))["iterations"]) >= 2
    with engine(p) as fresh:
        assert solve(fresh, p, 3) == want
