"""-m gpu: the exact bits of pba_covariance and pba_marginalize on a fixed list of small windows, pinned to a recording
(tests/golden/elimination_bits.json).

The covariance and marginalisation suites compare the two calls with extended-precision references under tolerances, so they cannot see
a change that moves a result within its bar -- which is what an edit to the point elimination both calls share (csrc/pba_elim.h) may do.
This test compares the built library with what the library of an earlier commit (the fixture's `commit` field) returned on an MI355X:
per case the status, every field of the info struct as hex floats and the SHA-1 of every output array, field by field; after
PBA_ERR_NUMERIC the SHA-1 of the poisoned caller buffers, which keep their bytes.  The cases and the recorder are
tools/ab_elimination_bits.py; one child process, the default driver.

A pull request that changes a summation order (or anything else that moves result bits) ON PURPOSE regenerates the fixture with
`python tools/ab_elimination_bits.py --out tests/golden/elimination_bits.json --commit <its hash>` and says so; any other mismatch here
is a bug."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("ab_elimination_bits", os.path.join(ROOT, "tools", "ab_elimination_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

with open(os.path.join(ROOT, "tests", "golden", "elimination_bits.json")) as _f:
    GOLDEN = json.load(_f)


def _fields(name, rec):
    return bits.FIELDS[name.split("/")[0]] + (bits.FAILURE_FIELDS if rec["status"] == bits.PBA_ERR_NUMERIC else ())


def test_fixture_holds_every_case():
    """The recording names its commit and holds exactly the recorder's cases and fields; the two point failures are numeric errors that
    name point 37 and left the caller's buffers alone, and every other case but the open gauge succeeded."""
    assert len(GOLDEN["commit"]) == 40
    recs = GOLDEN["cases"]
    assert sorted(recs) == sorted(bits.case_names())
    assert len([n for n in recs if n.startswith("marg/")]) == 22 + 2
    for name, c in recs.items():
        assert sorted(c) == sorted(_fields(name, c)), name
        assert c["status"] in (0, bits.PBA_ERR_NUMERIC), name
        if c["status"] == bits.PBA_ERR_NUMERIC:
            assert c["kept"] is True, name
        elif name != "cov/fail/5x60-causal-huber-anchor-0":
            assert c["failed_index"] == -1, name
    for name in ("cov/fail/single-observation", "marg/fail/point"):
        c = recs[name]
        assert c["status"] == bits.PBA_ERR_NUMERIC and c["failed_is_point"] == 1 and c["failed_index"] == bits.VICTIM
    assert all(c["status"] == 0 for n, c in recs.items() if "/fail/" not in n)


@pytest.mark.gpu
def test_elimination_bits():
    want = GOLDEN["cases"]
    got = bits.record()
    assert sorted(got) == sorted(bits.case_names())
    bad = []
    for name in sorted(want):
        if sorted(got[name]) != sorted(want[name]):
            bad.append("%s: fields %r, recorded %r" % (name, sorted(got[name]), sorted(want[name])))
            continue
        bad += ["%s.%s: %r, recorded %r" % (name, f, got[name][f], want[name][f]) for f in sorted(want[name]) if got[name][f] != want[name][f]]
    assert not bad, "\n".join(bad)
