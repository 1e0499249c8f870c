"""`trainstep.SceneStep` wires every step that can be constructed without a GPU as it did before its constructor,
`forward_backward`, `describe()` and the inference methods were split into named parts, and its two constructors refuse what they
refused, in the same words: tests/golden/step_wiring.json holds the record tests/golden/make_step_wiring_golden.py defines for
every case (written by the commit before that change, never regenerated).  No GPU.  The `describe()` text is compared on its
own first, so that a slip there diffs as text."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_step_wiring_golden as G                             # noqa: E402

with open(G.PATH) as f:
    GOLDEN = json.load(f)
CASES, REFUSALS = G.all_cases(), G.refusals()


def test_the_cases_are_the_files():
    assert sorted(CASES) == sorted(GOLDEN["cases"]) and len(CASES) >= 28
    assert sorted(REFUSALS) == sorted(GOLDEN["refusals"]) and len(REFUSALS) >= 30
    assert all(v is not None for v in GOLDEN["refusals"].values())          # every one of them was refused
    assert not any("values" in rec for rec in GOLDEN["cases"].values())     # (machine-dependent: never in the committed file)
    assert "never regenerated" in GOLDEN["_header"]


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_the_step_is_wired_as_the_parent_wired_it(name):
    step = CASES[name]()
    rec = json.loads(json.dumps(G.record(step)))                # (through JSON: tuples and lists compare as the file holds them)
    want = GOLDEN["cases"][name]
    assert rec["describe"] == want["describe"]
    for key in G.LISTS:                                         # held as [length, digest]: a failure shows the list as it is now
        assert rec[key] == want[key], (key, G.record(step, full=True)[key])
    assert rec == want


@pytest.mark.parametrize("name", sorted(GOLDEN["refusals"]))
def test_the_constructors_refuse_in_the_parents_words(name):
    assert G.refusal_record(REFUSALS[name]) == GOLDEN["refusals"][name]
