"""-m gpu: the exact bits of a fixed list of small solves, pinned to a recording (tests/golden/solve_bits.json).

The batch = solo and resident = pipelined checks of the suite compare two paths of ONE build, so they cannot see a change that moves
both alike -- which is what an edit to a device body shared by the solo and the batched launches does.  This test compares the built
library with what the library of an earlier commit (the fixture's `commit` field) returned on an MI355X: per case the driver, the
hex iteration costs, the termination type and the SHA-1 of the cameras, of the points and of the observation records, field by
field.  The cases and the recorder are tools/ab_bits.py; one child process per environment, as the driver is chosen at pba_create.

A pull request that changes a summation order (or anything else that moves result bits) ON PURPOSE regenerates the fixture with
`python tools/ab_bits.py --out tests/golden/solve_bits.json --commit <its hash>` and says so; any other mismatch here is a bug."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("ab_bits", os.path.join(ROOT, "tools", "ab_bits.py"))
ab_bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab_bits)

with open(os.path.join(ROOT, "tests", "golden", "solve_bits.json")) as _f:
    GOLDEN = json.load(_f)

FIELDS = ("driver", "costs", "termination_type", "cams", "xyz", "rec")


def test_fixture_holds_every_case():
    """The recording names its commit and holds exactly the recorder's cases, and the three reduce + solve modes are three different
    ends: the iteration limit (iterations 0..3, no convergence), no iteration at all, and an early stop by the function tolerance."""
    assert len(GOLDEN["commit"]) == 40
    assert sorted(GOLDEN["cases"]) == sorted(ab_bits.ENVS)
    for env, recs in GOLDEN["cases"].items():
        assert sorted(recs) == sorted(ab_bits.case_names(env))
        for name, c in recs.items():
            assert sorted(c) == sorted(FIELDS), (env, name)
        for w in ab_bits.WINDOWS:
            limit, zero, ftol = (recs["rs_%s_%s" % (w, s)] for s in ("limit", "zero", "ftol"))
            assert len(limit["costs"]) == 4 and len(zero["costs"]) == 1
            assert limit["termination_type"] == zero["termination_type"] != ftol["termination_type"]
            assert 1 < len(ftol["costs"]) < 51          # stopped by the tolerance, well before the default limit of 50 iterations


@pytest.mark.gpu
@pytest.mark.parametrize("env", sorted(ab_bits.ENVS))
def test_solve_bits(env):
    want = GOLDEN["cases"][env]
    got = ab_bits.record_env(env)
    assert sorted(got) == sorted(ab_bits.case_names(env))
    bad = ["%s.%s: %r, recorded %r" % (name, f, got[name][f], want[name][f]) for name in sorted(want) for f in FIELDS
           if got[name][f] != want[name][f]]
    assert not bad, "\n".join(bad)
