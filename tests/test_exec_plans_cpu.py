"""The step executor's plan compiler emits, for every unit form, storage mode and caller, the plans it emitted before the unit
description (`executor.Unit`) replaced the tagged block tuples: tests/golden/exec_plans.json holds one digest per stage of the
numbering-free record tests/golden/make_exec_plans_golden.py defines (written by the commit before that change, never
regenerated).  No GPU.  On a mismatch, diff `make_exec_plans_golden.py --full` of the two commits."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_exec_plans_golden as G                              # noqa: E402

with open(G.PATH) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def compiled():
    return {name: None if recs is None else [G.digest(r) for r in recs] for name, recs in G.all_cases()}


def test_the_cases_are_the_files(compiled):
    assert sorted(compiled) == sorted(GOLDEN)
    unet = [k for k in GOLDEN if k.startswith("unet/")]
    assert len(unet) == 44 and all(GOLDEN[k] for k in unet)
    assert sum(v is None for v in GOLDEN.values()) == 5 and all(k.startswith("refused/") for k, v in GOLDEN.items() if v is None)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_plans_are_the_parents(compiled, name):
    assert compiled[name] == GOLDEN[name]
