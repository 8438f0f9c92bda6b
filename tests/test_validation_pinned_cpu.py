"""Every call of tests/validation_cases.py is rejected as it was on the commit before the argument checks moved to
scene_utils/_args.py: the same exception class, the same message byte for byte (tests/golden/validation_parent.json), before the
native library is loaded.  And the table leaves out no `raise` of the walked modules except those that depend on what a kernel
wrote: the unreached ones, then and now, are exactly validation_cases.EXPECTED_UNCOVERED."""
import json

import pytest

import validation_cases as V

with open(V.GOLDEN) as f:
    PARENT = json.load(f)


def test_table_is_the_recorded_one():
    assert sorted(case[0] for case in V.CASES) == sorted(PARENT["cases"])


@pytest.fixture(scope="module")
def run():
    return V.run_all()


def test_rejections_are_the_parents(run):
    results, _ = run
    wrong = {k: (v, PARENT["cases"][k]) for k, v in results.items() if v != PARENT["cases"][k]}
    assert not wrong, "\n".join(f"{k}: now {v[0]}, the parent {v[1]}" for k, v in sorted(wrong.items()))


def test_unreached_raises_are_the_expected_ones(run):
    expected = sorted([fn, n] for fn, (n, why) in V.EXPECTED_UNCOVERED.items())
    assert all(why for _, why in V.EXPECTED_UNCOVERED.values())
    assert PARENT["uncovered"] == expected      # on the parent
    assert run[1] == expected                   # on this tree
