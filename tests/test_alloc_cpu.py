"""One owner for the handles' device and pinned memory, without a device.

  * The allocation registry (photobundle_amd/csrc/pba_alloc.h) is plain C++: tests/native/alloc_probe.cpp runs it over a malloc-backed
    backend that counts its calls.  The program is built here with AddressSanitizer + UBSan and run as a child process, one case per
    run; the leak checker at its exit speaks for the registry.  No sanitizer runtime is ever loaded into this interpreter.
  * The runtime's allocation, free and event calls are written in pba_handle.h alone (pba_comm.cpp keeps its peer-lifetime buffers), so
    "nothing leaks" is a property of that file: no other product source names them.
  * A failed create call of one matcher leaves the other matcher's create-error text alone.
"""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photobundle_amd", "csrc")
CASES = ["first_reserve", "zero_elements", "smaller_keeps", "larger_regrows", "mapped_view", "failure_mid_growth", "release_all_reuse",
         "abandon_frees_nothing"]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("alloc_probe") / "alloc_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "native", "alloc_probe.cpp")])
    return exe


def test_probe_knows_exactly_these_cases(probe):
    r = subprocess.run([probe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stdout.split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_registry(probe, case):
    r = subprocess.run([probe, case], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, (r.returncode, r.stdout, r.stderr)


def test_only_the_handle_header_calls_the_runtime_allocator():
    owned = re.compile(r"\b(hipMalloc|hipHostMalloc|hipFree|hipHostFree|hipEventCreate\w*|hipEventDestroy)\b")
    files = sorted(f for f in glob.glob(os.path.join(CSRC, "*")) if os.path.basename(f) not in ("pba_handle.h", "pba_comm.cpp"))
    assert len(files) >= 18
    for f in files:
        for k, line in enumerate(open(f).read().split("\n"), 1):
            assert not owned.search(line), "%s:%d names %s: allocations and events go through pba_handle.h" % (
                os.path.relpath(f, ROOT), k, owned.search(line).group(0))
    assert len(set(owned.findall(open(os.path.join(CSRC, "pba_handle.h")).read()))) >= 6      # (the pattern still finds them there)


def test_create_error_texts_are_per_handle_type():
    """Both create calls validate before touching a device: an invalid create of one matcher sets its own text only."""
    from photobundle_amd import stereo
    L = stereo._stereo_lib()
    stereo._sgm_lib()
    out = C.c_void_p()
    bm_bad, sgm_bad = stereo.default_params(number_of_disparities=24), stereo.sgm_default_params(number_of_disparities=16, census_radius=3)
    assert L.pba_sgm_create(40, 64, C.byref(sgm_bad), 0, C.byref(out)) == -1 and not out.value
    sgm_text = L.pba_sgm_last_error(None)
    assert b"censusRadius" in sgm_text
    assert L.pba_stereo_create(40, 64, C.byref(bm_bad), 0, C.byref(out)) == -1 and not out.value
    bm_text = L.pba_stereo_last_error(None)
    assert b"numberOfDisparities" in bm_text
    assert L.pba_sgm_last_error(None) == sgm_text                    # ... unchanged by the stereo failure
    sgm_bad2 = stereo.sgm_default_params(number_of_disparities=16, window_radius=10)
    assert L.pba_sgm_create(40, 64, C.byref(sgm_bad2), 0, C.byref(out)) == -1 and not out.value
    assert b"windowRadius" in L.pba_sgm_last_error(None)
    assert L.pba_stereo_last_error(None) == bm_text                  # ... and the other way round
