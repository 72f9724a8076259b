"""The feature-conflict table of photobundle_amd/csrc/pba_mode_rules.h, compiled stand-alone (tests/mode_rules_probe.cpp): every
ordered pair of features against the sentences the refusal sites of pba_engine.hip spelled out before the table existed (copied
from that source, word for word), null for every other pair, symmetry of the conflicts, and the order of the answers where several
conflicts are present at once (the order of the checks at each site before the table)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MULTI, INVDEPTH, SWEEP, WIDE, PTS, CAMS, ANCHORS, COV, BATCH = (1 << k for k in range(9))
FEATURES = (MULTI, INVDEPTH, SWEEP, WIDE, PTS, CAMS, ANCHORS, COV, BATCH)

SWEEP_MODES = "the precision-sweep sampler modes (pba_config.flags bits 1-2) "

# (feature present, feature switched on) -> the sentence of the site that switches it on
EXPECTED = {
    # wide_refusal (pba_set_cameras / pba_set_cameras_anchored on a wide window)
    (MULTI, WIDE): "multi-rank solves (pba_comm_*) are not built for wide windows",
    (INVDEPTH, WIDE): "the inverse-depth mode (pba_set_inverse_depth) is not built for wide windows",
    (SWEEP, WIDE): SWEEP_MODES + "are not built for wide windows",
    # anchors_refusal (two or more constant slots)
    (MULTI, ANCHORS): "multi-rank solves (pba_comm_*) take at most one constant slot",
    (SWEEP, ANCHORS): SWEEP_MODES + "take at most one constant slot",
    # pba_set_inverse_depth
    (WIDE, INVDEPTH): "the inverse-depth mode is not built for wide windows",
    # pose_refusal + pba_set_points_constant
    (MULTI, PTS): "multi-rank solves (pba_comm_*) are not built for the points-constant mode",
    (SWEEP, PTS): SWEEP_MODES + "are not built for the points-constant mode",
    (CAMS, PTS): "the cameras-constant mode (pba_set_cameras_constant) is on: with every block constant the program is empty",
    # points_refusal (pba_set_cameras_constant)
    (PTS, CAMS): "the points-constant mode (pba_set_points_constant) is on: with every block constant the program is empty",
    (MULTI, CAMS): "multi-rank solves (pba_comm_*) are not built for the cameras-constant mode",
    (SWEEP, CAMS): SWEEP_MODES + "are not built for the cameras-constant mode",
    # pba_comm_init_rccl / pba_comm_init_callback
    (WIDE, MULTI): "multi-rank solves are not built for wide windows",
    (PTS, MULTI): "multi-rank solves are not built for the points-constant mode (pba_set_points_constant)",
    (CAMS, MULTI): "multi-rank solves are not built for the cameras-constant mode (pba_set_cameras_constant)",
    (ANCHORS, MULTI): "multi-rank solves take at most one constant slot",
    # pba_covariance
    (MULTI, COV): "multi-rank engines (pba_comm_*) are not built for the covariance output",
    (SWEEP, COV): SWEEP_MODES + "are not built for the covariance output",
    (INVDEPTH, COV): "the inverse-depth mode (pba_set_inverse_depth) with free cameras is not built; the cameras-constant mode takes it",
    # pba_internal_batch_validate
    (MULTI, BATCH): "multi-rank engines (pba_comm_*) solve alone",
    (WIDE, BATCH): "wide window",
    (SWEEP, BATCH): "the precision-sweep flags solve alone",
    (PTS, BATCH): "the points-constant mode (pba_set_points_constant) solves alone",
    (CAMS, BATCH): "the cameras-constant mode (pba_set_cameras_constant) solves alone",
}
# The sampler flags are fixed at pba_create, the covariance output and a batch are calls: nothing is ever switched on next to them, and
# no site held a sentence for that order.  The table answers with the sentence of the order that exists.
ONE_WAY = (SWEEP, COV, BATCH)


@pytest.fixture(scope="module")
def lookup(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("mode_rules")), "mode_rules_probe")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "mode_rules_probe.cpp")])

    def run(queries):
        r = subprocess.run([exe], input="".join("%x %x\n" % q for q in queries), capture_output=True, text=True, check=True, timeout=60)
        out = [line.split("\t") for line in r.stdout.splitlines()]
        assert len(out) == len(queries)
        return [(int(w, 16), None if s == "-" else s) for w, s in out]
    return run


PAIRS = [(a, b) for a in FEATURES for b in FEATURES]


def test_there_are_24_sentences():
    assert len(EXPECTED) == 24 and len(set(EXPECTED.values())) == 24


def test_every_pair_in_both_orders(lookup):
    got = dict(zip(PAIRS, lookup(PAIRS)))
    for (present, on), (with_, why) in got.items():
        want = EXPECTED.get((present, on))
        if want is None and (on in ONE_WAY or present in ONE_WAY):
            want = EXPECTED.get((on, present))
        assert why == want, (hex(present), hex(on), why)
        assert with_ == (present if want else 0)


def test_a_pair_conflicts_in_one_order_iff_in_the_other(lookup):
    got = dict(zip(PAIRS, lookup(PAIRS)))
    for a, b in PAIRS:
        assert (got[(a, b)][1] is None) == (got[(b, a)][1] is None), (hex(a), hex(b))
    assert all(got[(a, a)][1] is None for a in FEATURES)
    assert sum(why is not None for _, why in got.values()) == 2 * 18      # 10 pairs of states, 3 + 5 of the two calls


@pytest.mark.parametrize("present,on,first", [
    (MULTI | INVDEPTH | SWEEP, WIDE, MULTI), (INVDEPTH | SWEEP, WIDE, INVDEPTH),           # wide_refusal: multi, inverse depth, sweep
    (MULTI | SWEEP, ANCHORS, MULTI), (MULTI | SWEEP, PTS, MULTI), (MULTI | SWEEP, CAMS, MULTI),
    (WIDE | PTS | ANCHORS, MULTI, WIDE), (PTS | ANCHORS, MULTI, PTS), (CAMS | ANCHORS, MULTI, CAMS), (WIDE | CAMS, MULTI, WIDE),
    (MULTI | SWEEP | INVDEPTH, COV, MULTI), (SWEEP | INVDEPTH, COV, SWEEP),               # pba_covariance: multi, sweep, inverse depth
    (MULTI | SWEEP, BATCH, MULTI), (WIDE | PTS, BATCH, WIDE), (WIDE | CAMS, BATCH, WIDE),
])
def test_several_conflicts_are_reported_in_the_order_of_the_old_checks(lookup, present, on, first):
    """Only sets of features that can be present together are asked (features that exclude each other never are)."""
    (with_, why), = lookup([(present, on)])
    assert with_ == first and why == EXPECTED[(first, on)]


def test_features_that_do_not_conflict_are_ignored(lookup):
    (with_, why), = lookup([(INVDEPTH | ANCHORS | WIDE | PTS, CAMS)])
    assert with_ == PTS and why == EXPECTED[(PTS, CAMS)]
    assert lookup([(INVDEPTH | ANCHORS | WIDE, CAMS), (0, WIDE), (MULTI | INVDEPTH | SWEEP, INVDEPTH)]) == [(0, None)] * 3


def test_the_sentences_live_in_the_header_alone():
    with open(os.path.join(ROOT, "photobundle_amd", "csrc", "pba_engine.hip")) as f:
        src = f.read()
    for why in EXPECTED.values():
        if why != "wide window":      # (two words the engine's comments use too)
            assert why not in src, why
