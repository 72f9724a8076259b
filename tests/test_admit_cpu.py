"""CPU side of the re-observation (include/pba.h "re-observation"): the ABI, the numpy restatement of the rule against hand-written
cases, the merged lists, the two rows of the feature-conflict table, the class's four keys, and the host bookkeeping as a stand-alone
program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import admit_cases as ac
from photobundle_amd import _lib, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_mirrored():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "pba.h")).read()
    assert re.search(r"int\s+pba_admit\s*\(\s*pba_engine\s*\*\s*e\s*,\s*const\s+pba_admit_options\s*\*\s*o\s*,\s*int32_t\s+capacity\s*,[^;]*"
                     r"int32_t\s*\*\s*cand_point\s*,\s*int32_t\s*\*\s*cand_slot\s*,\s*double\s*\*\s*cand_cost\s*,\s*uint8_t\s*\*\s*cand_take[^;]*"
                     r"pba_admit_info\s*\*\s*info[^;]*\)\s*;", header)
    assert hasattr(L, "pba_admit") and "pba_admit" in _lib.SYMBOLS
    assert [f for f, _ in _lib.AdmitOptions._fields_] == ["slot_mask", "min_depth", "border", "min_cost", "factor", "quantile", "apply"]
    assert [f for f, _ in _lib.AdmitInfo._fields_] == ["n_blocks_before", "n_blocks_after", "n_points", "n_candidates", "n_admitted", "n_written",
                                                      "quantile_cost", "threshold", "applied"]


def test_struct_layout_matches_the_header():
    fields_o = [f for f, _ in _lib.AdmitOptions._fields_]
    fields_i = [f for f, _ in _lib.AdmitInfo._fields_]
    src = ('#include "pba.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) { printf("%zu %zu", sizeof(pba_admit_options), sizeof(pba_admit_info));\n' +
           "".join('printf(" %%zu", offsetof(pba_admit_options, %s));\n' % f for f in fields_o) +
           "".join('printf(" %%zu", offsetof(pba_admit_info, %s));\n' % f for f in fields_i) + 'printf("\\n"); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), c])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    O, I = _lib.AdmitOptions, _lib.AdmitInfo
    assert got == [C.sizeof(O), C.sizeof(I)] + [getattr(O, f).offset for f in fields_o] + [getattr(I, f).offset for f in fields_i]


def test_null_arguments_are_refused_without_a_device():
    L = _lib.lib()
    o, info = _lib.AdmitOptions(1, 0.1, 1, 0.0, 1.0, 0.5, 0), _lib.AdmitInfo()
    assert L.pba_admit(None, C.byref(o), 0, None, None, None, None, C.byref(info)) == -1       # PBA_ERR_INVALID


# ---- the rule, by hand ---------------------------------------------------------------------------------------------------------------
def _admit(c, cand, **kw):
    take, info = ac.reference_admit(np.array(c, np.float64), np.array(cand, np.float64), **kw)
    return list(take), info


def test_a_tie_at_the_threshold_is_taken():
    existing = [1.0, 2.0, 3.0, 4.0, 5.0]      # k = floor(0.5 * 4) = 2 -> 3.0
    take, info = _admit(existing, [3.0, np.nextafter(3.0, 4.0), np.nextafter(3.0, 0.0), 0.0], factor=1.0, quantile=0.5)
    assert info["quantile_cost"] == 3.0 and info["threshold"] == 3.0 and take == [1, 0, 1, 1]
    assert info["n_candidates"] == 4 and info["n_admitted"] == 3 and info["n_blocks_before"] == 5 and info["n_blocks_after"] == 8
    # ... and through the floor: min_cost above factor x quantile
    take, info = _admit(existing, [3.5, np.nextafter(3.5, 4.0)], min_cost=3.5, factor=1.0, quantile=0.5)
    assert info["threshold"] == 3.5 and take == [1, 0]


def test_nan_and_inf_candidates_are_never_taken():
    take, info = _admit([1.0, 2.0], [NAN, INF, -INF, 1e300, 0.5], min_cost=1e300, factor=0.0)
    assert take == [0, 0, 1, 1, 1] and info["n_admitted"] == 3      # (-inf <= t holds; a cost is never negative, the rule does not care)
    take, _ = _admit([1.0, 2.0], [NAN, INF], min_cost=0.0, factor=1.0, quantile=1.0)
    assert take == [0, 0]


def test_factor_zero_ignores_the_quantile():
    take, info = _admit([4.0, 1.0, 3.0, INF], [2.9, 3.0, 3.1], min_cost=3.0, factor=0.0, quantile=1.0)
    assert info["threshold"] == 3.0 and info["quantile_cost"] == INF and take == [1, 1, 0]
    # threshold 0: only a cost of exactly zero is taken
    take, info = _admit([4.0, 1.0], [0.0, 5e-324, 1.0], min_cost=0.0, factor=0.0)
    assert info["threshold"] == 0.0 and take == [1, 0, 0]


def test_quantile_zero_and_one_run_over_the_existing_blocks_only():
    existing = [4.0, 1.0, 3.0, 2.0]
    cand = [0.5, 1.0, 2.5, 4.0, 9.0]
    lo, hi = _admit(existing, cand, factor=1.0, quantile=0.0), _admit(existing, cand, factor=1.0, quantile=1.0)
    assert lo[1]["quantile_cost"] == 1.0 and lo[0] == [1, 1, 0, 0, 0] and hi[1]["quantile_cost"] == 4.0 and hi[0] == [1, 1, 1, 1, 0]
    # k = floor(q (n - 1)) with n the EXISTING blocks: 0.34 * 3 = 1.02 -> 1, 0.33 * 3 = 0.99 -> 0
    assert _admit(existing, cand, quantile=0.34)[1]["quantile_cost"] == 2.0 and _admit(existing, cand, quantile=0.33)[1]["quantile_cost"] == 1.0
    # no candidates at all: counts of nothing
    take, info = _admit(existing, [], quantile=0.5)
    assert take == [] and info["n_candidates"] == 0 and info["n_blocks_after"] == 4


def test_the_non_finite_product():
    with pytest.raises(ac.AdmitNumericError):
        _admit([1.0, INF], [1.0], factor=1.0, quantile=1.0)
    with pytest.raises(ac.AdmitNumericError):
        _admit([1.0, NAN], [1.0], factor=2.0, quantile=1.0)       # NaN orders last
    with pytest.raises(ac.AdmitNumericError):
        _admit([1e308, 1e308], [1.0], factor=10.0, quantile=0.0)  # overflow
    assert _admit([1.0, INF], [1.0], factor=0.0, quantile=1.0, min_cost=2.0)[0] == [1]      # factor 0 never multiplies


# ---- the candidates and the merged lists -------------------------------------------------------------------------------------------------
def test_candidates_by_hand():
    from photobundle_amd.problem import WindowProblem
    # two cameras at the origin looking down z (identity poses), K = (128, 128, 50, 40), 80 x 100 images
    planes = np.zeros((2, 3, 80, 100), np.float32)
    xyz = np.array([[0.0, 0.0, 2.0],        # u = 50, v = 40: inside
                    [-0.765625, 0.0, 2.0],  # u = 1: on the bound of border 1, outside border 2
                    [0.0, 0.0, 0.05],       # too close for min_depth 0.1
                    [0.0, 0.0, -1.0],       # behind
                    [NAN, 0.0, 2.0]])       # non-finite
    p = WindowProblem(K=(128.0, 128.0, 50.0, 40.0), radius=1, planes=planes, cams=np.zeros((2, 6)), xyz=xyz, desc=np.zeros((5, 9)),
                      obs_point=np.arange(5, dtype=np.int32), obs_slot=np.zeros(5, np.int32), weights=np.ones(9))
    cp, cs, _ = ac.reference_candidates(p, p.cams, xyz, 0b11, 0.1, 1)
    assert list(zip(cp, cs)) == [(0, 1), (1, 1)]
    cp, cs, _ = ac.reference_candidates(p, p.cams, xyz, 0b11, 0.1, 2)
    assert list(zip(cp, cs)) == [(0, 1)]
    assert len(ac.reference_candidates(p, p.cams, xyz, 0b01, 0.1, 1)[0]) == 0      # slot 0 holds every point already
    cp, cs, _ = ac.reference_candidates(p, p.cams, xyz, 0b10, 0.01, 1)
    assert list(zip(cp, cs)) == [(0, 1), (1, 1), (2, 1)]


@pytest.fixture(scope="module")
def holes():
    return ac.with_holes(synthetic.make_window(**ac.BASE))


def test_the_window_with_holes(holes):
    base = synthetic.make_window(**ac.BASE)
    assert base.n_obs == 800 and holes.n_points == 200 and 500 < holes.n_obs < 600
    assert (np.bincount(holes.obs_point, minlength=200) > 0).all()
    gone = set(zip(base.obs_point.tolist(), base.obs_slot.tolist())) - set(zip(holes.obs_point.tolist(), holes.obs_slot.tolist()))
    assert gone and all((a + b) % 3 == 0 for a, b in gone)


def test_merged_lists_pass_the_layout_checks(holes):
    p = holes
    cp, cs, margins = ac.reference_candidates(p, p.cams, p.xyz, 0b1111, 0.1, 1)
    assert margins["px"] > 1e-6 and margins["depth"] > 1e-9 and len(cp) > 100
    assert not (set(zip(cp.tolist(), cs.tolist())) & set(zip(p.obs_point.tolist(), p.obs_slot.tolist())))
    assert (np.diff(cp) >= 0).all() and (np.diff(cs)[np.diff(cp) == 0] > 0).all()
    rng = np.random.default_rng(3)
    for take in (np.zeros(len(cp), bool), np.ones(len(cp), bool), rng.random(len(cp)) < 0.5):
        mp, ms = ac.merged_lists(p.obs_point, p.obs_slot, cp, cs, take)
        assert len(mp) == p.n_obs + int(take.sum()) and ac.layout_errors(p.n_points, mp, ms, p.n_frames) == []
        assert (np.diff(mp) >= 0).all() and (np.diff(ms)[np.diff(mp) == 0] > 0).all()       # grouped, slots strictly ascending
        assert set(zip(mp.tolist(), ms.tolist())) == set(zip(p.obs_point.tolist(), p.obs_slot.tolist())) | set(zip(cp[take].tolist(), cs[take].tolist()))
    # the checks themselves notice what they are for
    assert ac.layout_errors(3, [0, 0, 2], [0, 1, 0], 4) == ["a point has no observation"]
    assert ac.layout_errors(2, [0, 0, 1], [1, 1, 0], 4) == ["duplicate / unsorted slot"]
    assert ac.layout_errors(2, [1, 0], [0, 0], 4) == ["observations must be grouped by point"]
    assert ac.layout_errors(2, [0, 1], [0, 4], 4) == ["observation out of range"]


# ---- the feature-conflict table ----------------------------------------------------------------------------------------------------------
MULTI, INVDEPTH, SWEEP, WIDE, PTS, CAMS, ANCHORS, COV, BATCH, PRIOR, CULL, ADMIT = (1 << k for k in range(12))
EARLIER = (MULTI, INVDEPTH, SWEEP, WIDE, PTS, CAMS, ANCHORS, COV, BATCH, PRIOR, CULL)
ADMIT_SENTENCES = {
    MULTI: "multi-rank engines (pba_comm_*) are not built for re-observation: the order statistic would need an exchange",
    SWEEP: "the precision-sweep sampler modes (pba_config.flags bits 1-2) are not built for re-observation",
}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("admit_mode_rules")), "admit_mode_rules_probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "admit_mode_rules_probe.cpp")])

    def run(queries):
        r = subprocess.run([exe], input="".join("%x %x\n" % q for q in queries), capture_output=True, text=True, check=True, timeout=60)
        lines = r.stdout.splitlines()
        head, out = lines[0].split("\t"), [line.split("\t") for line in lines[1:]]
        assert len(out) == len(queries)
        return head, [(int(w, 16), None if s == "-" else s, None if old == "-" else old) for w, s, old in out]
    return run


def test_the_two_rows_of_pba_admit_close_the_table(table):
    head, _ = table([])
    assert int(head[1], 16) == ADMIT == 2048
    assert [int(v, 16) for v in head[2].split()] == [MULTI, ADMIT] and [int(v, 16) for v in head[3].split()] == [SWEEP, ADMIT]
    # pba_admit asks with the engine's features present; the same sentence answers the other order (a call is never present)
    for other in EARLIER:
        want = ADMIT_SENTENCES.get(other)
        _, got = table([(other, ADMIT), (ADMIT, other)])
        assert [g[1] for g in got] == [want, want], other
        assert [g[0] for g in got] == ([other, ADMIT] if want else [0, 0])
    # several present: the multi-rank row comes first
    _, got = table([(MULTI | SWEEP | WIDE | PRIOR, ADMIT), (SWEEP | ANCHORS | INVDEPTH, ADMIT), (WIDE | ANCHORS | INVDEPTH | PTS | CAMS | PRIOR, ADMIT)])
    assert [g[1] for g in got] == [ADMIT_SENTENCES[MULTI], ADMIT_SENTENCES[SWEEP], None]


def test_no_earlier_answer_changed(table):
    # every set of earlier features present x every earlier feature switched on: the answer is the one the table gives without its last
    # two rows, and it never names pba_admit
    queries = [(present, on) for present in range(1 << len(EARLIER)) for on in EARLIER]
    _, got = table(queries)
    for q, (with_, sentence, old) in zip(queries, got):
        assert sentence == old and with_ != ADMIT, q
    assert sum(1 for g in got if g[1]) > 1000
    # ... also with the new bit among the present ones, wherever the earlier rows answer at all
    _, got = table([(present | ADMIT, on) for present, on in queries[::7]])
    assert all(s == old for _, s, old in got if old)


# ---- the class ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    import admit_class_probe
    return admit_class_probe.AdmitClassProbe(tmp_path_factory.mktemp("admit_probe"))


def test_option_fields_defaults_and_config_keys(probe):
    header = open(os.path.join(ROOT, "photobundle_amd", "host", "photobundle.h")).read()
    for field in ("int reobservePasses = 0;", "double reobserveFactor = 1.0;", "double reobserveQuantile = 0.5;", "double reobserveMinCost = 0.0;",
                  "int numAdmittedBlocks = 0;"):
        assert header.count(field) == 1, field
    assert probe.defaults() == ((0.0, 1.0, 0.5, 0.0), 0)
    text = probe.parse_and_print("slidingWindowSize = 4\n")
    for line in ("reobservePasses = 0\n", "reobserveFactor = 1\n", "reobserveQuantile = 0.5\n", "reobserveMinCost = 0\n"):
        assert line in text, line
    text = probe.parse_and_print("reobservePasses = 2\nreobserveFactor = 2.5\nreobserveQuantile = 0.75\nreobserveMinCost = 0.125\n")
    for line in ("reobservePasses = 2\n", "reobserveFactor = 2.5\n", "reobserveQuantile = 0.75\n", "reobserveMinCost = 0.125\n"):
        assert line in text, line
    assert probe.parse_and_print(text) == text      # the output of one run configures the next


def test_constructor_refuses_out_of_range_values(probe):
    size, K = (96, 128), (160.0, 160.0, 64.0, 48.0)
    for kw, match in ((dict(passes=-1), "reobservePasses = -1"), (dict(passes=1, quantile=1.5), "reobserveQuantile = 1.5"),
                      (dict(passes=1, quantile=NAN), "reobserveQuantile"), (dict(passes=1, factor=-1.0), "reobserveFactor = -1"),
                      (dict(passes=1, factor=INF), "reobserveFactor"), (dict(passes=1, min_cost=-0.5), "reobserveMinCost = -0.5"),
                      (dict(passes=1, min_cost=INF), "reobserveMinCost")):
        with pytest.raises(RuntimeError, match=match):
            probe.create(size, K, window=5, radius=1, **kw)


# ---- the host bookkeeping under the sanitizers -----------------------------------------------------------------------------------------------
def test_list_merging_and_visibility_bookkeeping_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "admit_lists_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "admit_lists_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-2000:])
