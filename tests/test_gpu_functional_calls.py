"""The convolution-type autograd nodes of functional.py hand the library the launches they handed it before their
parameter-gradient decision moved into one helper: tests/golden/functional_calls.json holds, for every node, storage type, bias,
switch setting and subset of requested gradients, the ordered library calls of a forward and backward -- entry point, integer
arguments, which pointers are NULL, and the kernel name and figures given to the timer (written by the commit before that change by
tests/golden/make_functional_calls_golden.py, never regenerated)."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_functional_calls_golden as G                        # noqa: E402

pytestmark = pytest.mark.gpu

with open(G.PATH) as f:
    GOLDEN = json.load(f)["cases"]

_SCENE = []


def _scene(gpu):
    if not _SCENE:
        _SCENE.append(G.Scene(gpu))
        _SCENE.append(G.all_cases(_SCENE[0]))
    return _SCENE[0]


def _cases(gpu):
    _scene(gpu)
    return _SCENE[1]


def test_the_golden_holds_exactly_the_cases_the_maker_defines(gpu):
    cases = _cases(gpu)
    assert sorted(cases) == sorted(GOLDEN)
    assert all(any(name.startswith(g + "/") for g in G.GROUPS) for name in cases)


@pytest.mark.parametrize("group", G.GROUPS)
def test_a_node_makes_the_library_calls_of_the_golden(gpu, group):
    cases = _cases(gpu)
    names = [n for n in cases if n.startswith(group + "/")]
    assert names
    wrong = {}
    for name in names:
        calls = G.run_case(cases[name])
        if calls != GOLDEN[name]:
            wrong[name] = (calls, GOLDEN[name])
    assert not wrong, "\n".join(f"{n}:\n  got      {g}\n  expected {e}" for n, (g, e) in wrong.items())


@pytest.mark.parametrize("variant", ["bias-pair1", "bias-pair0", "nobias-pair1", "nobias-pair0"])
def test_the_one_residual_node_takes_bf16_features_with_the_calls_of_the_bf16_name(gpu, variant):
    """`ResidualBlockFunction` dispatches on the features' storage type (modules.Sequential hands it both): on bf16-stored features
    it makes the calls the golden holds for `ResidualBlockFunctionBF16`."""
    from sparse_rcnn_amd import functional as F
    scene, cases = _scene(gpu), _cases(gpu)
    one = lambda i: F.ResidualBlockFunction.apply(i["x"], i["w1"], i.get("b1"), i["w2"], i.get("b2"), scene.md, scene.size)
    names = [n for n in cases if n.startswith(f"residual/bf16/{variant}/")]
    assert names
    for name in names:
        switches, inputs, _, want = cases[name]
        assert G.run_case((switches, inputs, one, want)) == GOLDEN[name], name


def test_the_bf16_name_of_the_residual_node_refuses_fp32_features(gpu):
    from sparse_rcnn_amd import _lib as L, functional as F
    scene, cases = _scene(gpu), _cases(gpu)
    _, i, _, _ = cases["residual/f32/bias-pair1/x"]
    with pytest.raises(L.ScnError, match="ResidualBlockFunctionBF16 takes torch.bfloat16 features"):
        F.ResidualBlockFunctionBF16.apply(i["x"], i["w1"], i["b1"], i["w2"], i["b2"], scene.md, scene.size)
    with pytest.raises(TypeError, match="compute in fp32"):
        F.ResidualBlockFunction.apply(i["x"].half(), i["w1"], i["b1"], i["w2"], i["b2"], scene.md, scene.size)
    with pytest.raises(L.ScnError, match="multiples of 8"):
        F.ResidualBlockFunction.apply(i["x"].to(torch.bfloat16)[:, :12], i["w1"], i["b1"], i["w2"], i["b2"], scene.md, scene.size)
