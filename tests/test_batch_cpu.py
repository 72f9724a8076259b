"""CPU checks of the batched solve's C-ABI (pba_solve_batch): declared, exported, and argument errors refused before any device call."""
import ctypes as C
import os
import re

import pytest

from photobundle_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_batch_entry_and_its_limit():
    header = open(os.path.join(ROOT, "include", "pba.h")).read()
    assert re.search(r"#define\s+PBA_MAX_BATCH\s+64\b", header)
    assert re.search(r"int\s+pba_solve_batch\s*\(\s*pba_engine\s*\*\s*const\s*\*\s*engines\s*,\s*int32_t\s+n\s*,", header)
    assert _lib.MAX_BATCH == 64
    assert "pba_solve_batch" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "pba_solve_batch")


@pytest.mark.parametrize("n", [0, 65])
def test_batch_sizes_out_of_range_are_refused(n):
    L = _lib.lib()
    engines = (C.c_void_p * max(n, 1))()
    sums = (_lib.SolverSummary * max(n, 1))()
    assert L.pba_solve_batch(engines, n, None, sums, None, 0) == -1      # PBA_ERR_INVALID


def test_null_arguments_are_refused():
    L = _lib.lib()
    sums = (_lib.SolverSummary * 2)()
    assert L.pba_solve_batch(None, 2, None, sums, None, 0) == -1
    assert L.pba_solve_batch((C.c_void_p * 2)(None, None), 2, None, sums, None, 0) == -1
    assert L.pba_solve_batch((C.c_void_p * 2)(None, None), 2, None, None, None, 0) == -1


def test_solve_batch_of_nothing_raises():
    with pytest.raises(engine.EngineError, match="0 engines"):
        engine.solve_batch([])
    with pytest.raises(engine.EngineError, match="65 engines"):
        engine.solve_batch([object()] * 65)


RUN = os.path.join(ROOT, "photobundle_amd", "bin", "run_kitti")


@pytest.mark.parametrize("args,msg", [
    (["-b", "only-a-config.cfg"], "CONFIG:OUTPUT"),
    (["-b", "a.cfg:"], "CONFIG:OUTPUT"),
    (["-b", "a.cfg:out.txt:res.txt:extra"], "CONFIG:OUTPUT"),
    (["-b", "a.cfg:out.txt", "-c", "b.cfg"], "does not combine"),
    (["-o", "out.txt", "-b", "a.cfg:out2.txt"], "does not combine"),
    (["-b"], "usage"),
])
def test_run_kitti_refuses_a_bad_batch_before_any_device_call(args, msg, tmp_path):
    import subprocess
    assert os.path.exists(RUN), "build photobundle_amd/bin/run_kitti first (__graft_entry__.build())"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")       # nothing may reach a device: none is visible
    r = subprocess.run([RUN] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path), env=env)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert msg in r.stderr, r.stderr
    assert not os.listdir(str(tmp_path))
