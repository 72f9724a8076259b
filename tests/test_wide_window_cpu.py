"""CPU checks of the wide-window contract (windows of 16 to 32 free cameras, DESIGN.md "Wide windows"): pba_create takes up to
PBA_MAX_FRAMES = 32 slots and refuses 33 before any device call, the public header says so, and the dense numpy referee of the
GPU tests (tests/gpu_util.py) agrees with the oracle on a 24-frame window."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PBA_OK, PBA_ERR_INVALID, PBA_ERR_NO_DEVICE = 0, -1, -3


def _create(max_frames, **kw):
    from photobundle_amd import _lib
    L = _lib.lib()
    cfg = _lib.Config()
    cfg.rows, cfg.cols, cfg.max_frames, cfg.radius = 48, 64, int(max_frames), kw.get("radius", 2)
    cfg.fx, cfg.fy, cfg.cx, cfg.cy = 50.0, 50.0, 32.0, 24.0
    cfg.channels = kw.get("channels", 1)
    h = C.c_void_p()
    rc = L.pba_create(C.byref(cfg), C.byref(h))
    if h:
        L.pba_destroy(h)
    return rc


@pytest.mark.parametrize("max_frames", [17, 24, 32])
def test_create_accepts_up_to_32_slots(max_frames):
    import torch
    rc = _create(max_frames)
    assert rc != PBA_ERR_INVALID
    assert rc == (PBA_OK if torch.cuda.is_available() else PBA_ERR_NO_DEVICE)


@pytest.mark.parametrize("max_frames", [33, 64])
def test_create_refuses_33_slots_before_the_device(max_frames):
    assert _create(max_frames) == PBA_ERR_INVALID
    assert _create(max_frames, channels=3) == PBA_ERR_INVALID


def test_header_states_32():
    src = open(os.path.join(ROOT, "include", "pba.h")).read()
    assert re.search(r"#define\s+PBA_MAX_FRAMES\s+32\b", src)


def test_dense_referee_matches_the_oracle_on_a_24_frame_window():
    """gpu_util.dense_system / reference_step are the referee of the wide GPU tests: at 24 frames (23 free cameras, n = 138)
    their gradient and cost equal oracle.linearize and their first LM step equals iteration 1 of oracle.solve."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_util
    from oracle import oracle
    from photobundle_amd import synthetic
    p = synthetic.make_window(n_frames=24, n_points=60, radius=1, size=(96, 128), K=(150.0, 150.0, 64.0, 48.0),
                              visibility="causal", huber=0.05, seed_offset=3)
    assert p.n_frames == 24 and len(np.unique(p.obs_slot)) == 24
    J, r, n_cam = gpu_util.dense_system(p)
    assert n_cam == 6 * 23
    lin = oracle.linearize(p)
    free = [c for c in range(p.n_frames) if c != p.fixed_slot]
    g = J.T @ r
    assert np.allclose(g[:n_cam], lin["grad_cams"][free].reshape(-1), rtol=1e-10, atol=1e-10 * np.abs(g).max())
    assert np.allclose(g[n_cam:], lin["grad_pts"].reshape(-1), rtol=1e-10, atol=1e-10 * np.abs(g).max())
    rho = [2 * p.huber * np.sqrt(q) - p.huber ** 2 if q > p.huber ** 2 else q for q in lin["block_sqnorm"]]
    assert np.isclose(0.5 * sum(rho), lin["cost"], rtol=1e-12)
    ref = gpu_util.reference_step(J, r, n_cam, 1e4)
    assert ref["S"].shape == (n_cam, n_cam)
    res = oracle.solve(p, oracle.default_options(max_num_iterations=1))
    it = res["iterations"][1]
    assert np.isclose(it["step_norm"], np.linalg.norm(ref["delta"]), rtol=1e-8)
    assert np.isclose(it["model_cost_change"], ref["model_cost_change"], rtol=1e-8)
    assert np.isclose(res["iterations"][0]["gradient_max_norm"], np.abs(g).max(), rtol=1e-12)
