"""The reference's post-activation units, input-stage ReLUs and plain convolution blocks (unet.* with relu_first=,
drop_input_relu=, use_residuals=) without a GPU: the float64 restatement the GPU tests compare against
(tests/post_act_restate.py) meets fixtures the reference's own dense-mode factory produced; module trees and checkpoint key maps
equal the key lists of the reference's FeatureExtractor built with each switch setting; a reference-format state dict loads
completely; the step executor compiles plans for every form; the default network's plans are what they were; refusals; the new
executor op is declared and the library's entry points are the parent's."""
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # tests/post_act_restate.py, unit_forms_restate.py
import post_act_restate as R                                             # noqa: E402
from test_unit_forms_cpu import DEFAULT_PLAN_DIGESTS, _digest, _stages   # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# Both sides are float64 and the fixtures' operands are short dyadic numbers (make_post_act_golden.py): every sum is exact,
# whatever its order.  1e-12 of the tensor's scale is the bound the comparison is held to; observed: 0.
REL = 1e-12
SETTINGS = {"pre_keep": dict(drop_input_relu=False), "post_keep": dict(relu_first=False, drop_input_relu=False),
            "post_drop": dict(relu_first=False), "plain_pre": dict(use_residuals=False),
            "plain_post": dict(use_residuals=False, relu_first=False),
            "post_bottleneck": dict(relu_first=False, bottleneck_divisor=4),
            "post_mainpath_keep": dict(relu_first=False, drop_input_relu=False, main_path_relu=True)}
LEVELS = ["pre_keep", "post_keep", "post_drop", "plain_pre", "plain_post"]


def _rel(got, ref):
    return float((got.detach() - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def _leaves(P):
    return {k: v.clone().requires_grad_() for k, v in P.items()}


def _check_grads(out, dY, X, P, dX, G):
    names = sorted(P)
    assert sorted(G) == names
    grads = torch.autograd.grad(out, [X] + [P[k] for k in names], dY)
    assert _rel(grads[0], dX) <= REL
    for k, got in zip(names, grads[1:]):
        assert got.shape == G[k].shape and float(G[k].abs().max()) > 0 and _rel(got, G[k]) <= REL, k


def test_fixture_files_are_small():
    files = glob.glob(os.path.join(GOLD, "post_act_*"))
    assert len(files) == 2 + 10 + 1 + 1
    assert all(os.path.getsize(f) < 200_000 for f in files)


@pytest.mark.parametrize("name,C,d", [("plain", 16, 0), ("bottleneck", 32, 4)])
def test_restatement_meets_the_references_post_activation_unit(name, C, d):
    g = R.load(os.path.join(GOLD, f"post_act_unit_{name}.npz"))
    X, P, rules, n, flags, Y, dY, dX, G = R.fixture_unit(g)
    assert flags == dict(bottleneck_divisor=d, main_path_relu=False, relu_first=False, use_residuals=True)
    assert X.dtype == torch.float64 and X.shape == (2 * 8 * 8 * 4, C) and not bool(g["shimmed"])
    X, P = X.clone().requires_grad_(), _leaves(P)
    out = R.unit(X, P, "u", rules, n, **flags)
    assert _rel(out, Y) <= REL
    _check_grads(out, dY, X, P, dX, G)
    # the masks of its own ReLUs, prescribed through FrozenReLU, give the same function (the form the GPU tests use)
    from oracle import scn_oracle as O
    masks = []
    rec = lambda t: (masks.append(t.detach() > 0), torch.relu(t))[1]
    R.unit(X.detach(), {k: v.detach() for k, v in P.items()}, "u", rules, n, relu=rec, **flags)
    assert len(masks) == R.n_convs(d)                          # one ReLU per convolution: between them, and closing the branch
    fr = O.FrozenReLU(masks)
    again = R.unit(X, P, "u", rules, n, relu=fr, **flags)
    assert fr.k == len(masks) and torch.equal(again, out)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("name", LEVELS)
def test_restatement_meets_the_references_level(name, stride):
    g = R.load(os.path.join(GOLD, f"post_act_level_{name}_s{stride}.npz"))
    want = dict(relu_first=True, drop_input_relu=True, use_residuals=True)
    want.update(SETTINGS[name])
    assert {k: bool(g[k]) for k in want} == want and int(g["stride"]) == stride
    # the reference's get_units_level raises TypeError when an encoder level keeps its input ReLU: those fixtures needed the
    # generator's wrapper around get_activation (make_post_act_golden.py), the others ran the reference as it is
    assert bool(g["shimmed"]) == (not want["drop_input_relu"])
    X, P, G, Y, dY, dX = R.fixture_level(g)
    assert X.shape == (2 * 8 * 8 * 4 * stride ** 3, 8) and Y.shape == (2 * 8 * 8 * 4, 16)
    X, P = X.clone().requires_grad_(), _leaves(P)
    out = R.level_forward(g, X, P)
    assert _rel(out, Y) <= REL
    _check_grads(out, dY, X, P, dX, G)


def test_restatement_meets_the_references_decoder_level():
    g = R.load(os.path.join(GOLD, "post_act_reunite.npz"))
    Xc, S, P, G, Y, dY, dX, dS = R.fixture_reunite(g)
    assert Xc.shape == (512, 16) and S.shape == (4096, 8) and not bool(g["relu_first"])
    Xc, S, P = Xc.clone().requires_grad_(), S.clone().requires_grad_(), _leaves(P)
    out = R.reunite_forward(g, Xc, S, P)
    assert _rel(out, Y) <= REL
    names = sorted(P)
    grads = torch.autograd.grad(out, [Xc, S] + [P[k] for k in names], dY)
    assert _rel(grads[0], dX) <= REL and _rel(grads[1], dS) <= REL
    for k, got in zip(names, grads[2:]):
        assert _rel(got, G[k]) <= REL, k


def _keys():
    with open(os.path.join(GOLD, "post_act_keys.json")) as f:
        return json.load(f)


def _tree_keys(net):
    """state_dict keys of a SparseUNet under the reference's names: its module tree IS the reference's nesting, only the
    containers are named differently (encoder.<l> = main_network.<l>; decoder.<i>.up / nin / units = unet.module_list.<i>.
    input_stage / channel_changer / output_stage) and a bare input-stage layer stands for a Sequential of just it."""
    out = {}
    for k, v in net.state_dict().items():
        part = k.split(".")
        if part[0] == "encoder":
            rest = part[2:]
            if rest[0] == "0" and rest[1] in ("weight", "bias"):
                rest = ["0", "0"] + rest[1:]
            out[".".join(["main_network", part[1]] + rest)] = list(v.shape)
        else:
            name = {"up": "input_stage", "nin": "channel_changer", "units": "output_stage"}[part[2]]
            out[".".join(["unet.module_list", part[1], name] + part[3:])] = list(v.shape)
    return out


@pytest.mark.parametrize("name", list(SETTINGS))
def test_module_tree_and_key_map_equal_the_references_feature_extractor(name):
    from sparse_rcnn_amd.unet import SparseUNet, reference_key_map
    fx = _keys()[name]
    flags = SETTINGS[name]
    want = dict(relu_first=True, drop_input_relu=True, use_residuals=True, bottleneck_divisor=0, main_path_relu=False)
    want.update(flags)
    assert fx["flags"] == want
    kmap = reference_key_map(len(fx["channels"]), 2, **flags)
    assert sorted(kmap) == sorted(fx["keys"])
    net = SparseUNet(7, fx["channels"], **flags)
    assert _tree_keys(net) == fx["keys"]                      # the module tree itself, position by position
    own = net.named_oracle_params()
    assert sorted(own) == sorted(kmap.values())
    for rk, shape in fx["keys"].items():
        assert list(own[kmap[rk]].shape) == shape, rk
    assert sum(p.numel() for p in net.parameters()) == fx["n_params"]
    assert {k: tuple(p.shape) for k, p in own.items()} == dict(R.param_shapes(7, fx["channels"], **flags))


@pytest.mark.parametrize("name", list(SETTINGS))
def test_reference_state_dict_round_trip(name):
    from sparse_rcnn_amd.unet import Backbone, reference_key_map
    fx = _keys()[name]
    g = torch.Generator().manual_seed(3)
    sd = {}
    for k, shape in fx["keys"].items():                        # the reference's layout: grouped [fv, 1, nIn, nOut]
        t = torch.randn(shape, generator=g)
        sd["feature_extractor." + k] = t.unsqueeze(1) if len(shape) == 3 else t
    sd["rpn.head.weight"] = torch.zeros(3)                     # somebody else's tensor: neither missing nor unused
    net = Backbone(7, fx["channels"], **SETTINGS[name])
    assert net.load_reference_state_dict(sd) == ([], [])
    own = net.unet.named_oracle_params()
    for rk, name_ in reference_key_map(len(fx["channels"]), 2, **SETTINGS[name]).items():
        assert torch.equal(own[name_].detach(), sd["feature_extractor." + rk].reshape(own[name_].shape)), rk
    other = _keys()["plain_pre" if name != "plain_pre" else "pre_keep"]         # a checkpoint of ANOTHER form does not pass
    with pytest.raises((KeyError, ValueError)):
        net.load_reference_state_dict({"p." + k: torch.zeros(s) for k, s in other["keys"].items()})


@pytest.mark.parametrize("bf16", [False, "all"])
@pytest.mark.parametrize("name", list(SETTINGS))
def test_executor_plans_of_every_form(name, bf16):
    from sparse_rcnn_amd import _lib as L, executor as EX
    from sparse_rcnn_amd.unet import SparseUNet
    flags = SETTINGS[name]
    ch = (32, 64, 96, 128)
    net = SparseUNet(7, ch, bf16_blocks=bf16, **flags)
    stages = _stages(net)
    assert len(stages) == 4 + 3
    post = not flags.get("relu_first", True) and flags.get("use_residuals", True) and not flags.get("main_path_relu")
    seen = []
    for k, st in enumerate(stages):
        enc = k < 4
        for op in st.fwd + st.bwd:
            for field in ("x", "y", "r", "m", "x1", "y1"):
                assert -1 <= getattr(op, field) < len(st.bufs), field
        relus = [op for op in st.fwd if op.op == EX.OP_RELU]
        fused = [op for op in st.fwd if op.op == EX.OP_ADD_RELU]
        masks = [op for op in st.bwd if op.op == EX.OP_RELU_BWD]
        # the closing activation of a post-activation unit is ONE op with the skip's add; it leaves the branch slab alone
        assert len(fused) == (2 if post else 0)
        assert all(op.x1 not in (op.x, op.y) and op.r == -1 for op in fused)
        assert all(op.x == op.y for op in relus)                                      # in place
        # in-place SCN_OP_RELU: one behind the stage's layer (layer -> act), one behind every plain block / main-path unit
        relu_first = flags.get("relu_first", True)
        trail = int(not relu_first and (not enc or not flags.get("drop_input_relu", True)))
        closing = int(bool(flags.get("main_path_relu")) or (not flags.get("use_residuals", True) and not relu_first))
        assert len(relus) == trail + 2 * closing, (k, len(relus))
        assert len(masks) == len(relus) + len(fused)
        assert sorted(op.m for op in masks) == sorted([op.y for op in relus] + [op.x1 for op in fused])
        assert all(op.y not in (op.m, op.x1) and op.y != st.dout_id for op in masks)  # never into the incoming gradient
        # a stage whose last op is an in-place ReLU on its output, or whose backward masks by it, saves that output
        last = st.fwd[-1]
        ends_in_relu = last.op == EX.OP_RELU and last.y == st.out_id
        assert ends_in_relu == bool(closing)
        assert st.bwd_reads_out is ends_in_relu
        # a ReLU in front of a convolution stays in its gather, forward and weight gradient alike
        lead = sum(1 for op in st.fwd if op.op in (EX.OP_GEMM_IDENT, EX.OP_CONV_CHILD, EX.OP_RULES_CHILD) and op is st.fwd[0]
                   and op.flags & L.F_RELU_IN)
        assert lead == (1 if (flags.get("relu_first", True) and (not enc or not flags.get("drop_input_relu", True))) else 0)
        members = [m for reg in st.gregions for m in reg]
        assert len(members) == len(set(members)) == 2 * len(st.mods)
        assert len(st.lean_slot_of) == len(st.fwd_ws)
        slot = dict(zip(st.fwd_ws, st.lean_slot_of))
        for op in st.fwd:
            for out in (op.y, op.y1):
                for src in (op.x, op.r, op.m, op.x1):
                    if out in slot and src in slot and out != src:
                        assert slot[out] != slot[src], (op.op, out, src)
        seen += [m for m, _ in st.mods]
    convs = [m for m in net.modules() if hasattr(m, "weight") and hasattr(m, "nIn")]
    assert len(seen) == len(set(map(id, seen))) == len(convs)
    assert len(convs) == 4 + 3 * 2 + 7 * 2 * R.n_convs(flags.get("bottleneck_divisor", 0), flags.get("use_residuals", True))


@pytest.mark.parametrize("key", list(DEFAULT_PLAN_DIGESTS))
def test_default_plans_are_unchanged(key):
    from sparse_rcnn_amd.unet import SparseUNet
    ch, bf16 = key
    torch.manual_seed(0)
    plain = SparseUNet(7, ch, bf16_blocks=bf16)
    explicit = SparseUNet(7, ch, bf16_blocks=bf16, relu_first=True, drop_input_relu=True, use_residuals=True)
    assert _digest(explicit) == _digest(plain) == DEFAULT_PLAN_DIGESTS[key]
    assert repr(explicit) == repr(plain)
    assert list(explicit.state_dict()) == list(plain.state_dict())


def test_refusals_and_plumbing():
    from sparse_rcnn_amd.trainstep import SceneStep, SparseStepModel
    from sparse_rcnn_amd.unet import Backbone, SparseUNet, reference_key_map, units
    for bad in (dict(bottleneck_divisor=4), dict(main_path_relu=True)):
        with pytest.raises(ValueError, match="reference would ignore"):
            SparseUNet(7, (16, 32), use_residuals=False, **bad)
        with pytest.raises(ValueError, match="reference would ignore"):
            units(16, use_residuals=False, **bad)
        with pytest.raises(ValueError, match="reference would ignore"):
            reference_key_map(2, use_residuals=False, **bad)
    for flags in (dict(relu_first=False), dict(drop_input_relu=False), dict(use_residuals=False)):
        with pytest.raises(ValueError, match="bf16_blocks=True"):
            SparseUNet(7, (32, 64), bf16_blocks=True, **flags)
        with pytest.raises(ValueError, match="channel-padded"):
            SparseUNet(23, (23, 32), identity_first=True, **flags)
        SparseUNet(7, (32, 64), bf16_blocks="all", **flags)
    with pytest.raises(ValueError, match="multiples of 8"):
        SparseUNet(7, (16, 32), bf16_blocks="all", relu_first=False, bottleneck_divisor=4)
    # batch norm: the forms build (layer by layer; no plan)
    bn = SparseUNet(7, (16, 32), batchnorm=True, relu_first=False, drop_input_relu=False)
    assert not bn._exec_plan() and "BatchNormReLU" in repr(bn.encoder[1][0])
    assert not SparseUNet(7, (16, 32), batchnorm=True, use_residuals=False)._exec_plan()
    # the switches reach the step's backbone and its description
    m = SparseStepModel((16, 32), False, False, relu_first=False, drop_input_relu=False)
    u = m.backbone.unet
    assert (u.relu_first, u.drop_input_relu, u.use_residuals) == (False, False, True)
    assert Backbone(7, (16, 32)).unet.relu_first and Backbone(7, (16, 32), use_residuals=False).unet.use_residuals is False
    small = dict(device=torch.device("cpu"), channels=(16, 32), target=500, grid=(32, 32, 16), prefetch=False)
    st = SceneStep("cfg2", relu_first=False, drop_input_relu=False, **small)
    assert "relu_first=False" in st.describe() and "drop_input_relu=False" in st.describe()
    assert "use_residuals=False" in SceneStep("cfg2", use_residuals=False, **small).describe()
    d = SceneStep("cfg2", **small).describe()
    assert "relu_first" not in d and "use_residuals" not in d


def test_the_fused_op_is_an_executor_op_and_adds_no_entry_point():
    """The end of a post-activation unit is SCN_OP_ADD_RELU of scn_exec_run.  It has no entry point of its own: the set of
    entry points is the parent's (an existing test pins their number), so `scn_add_relu*` are neither declared nor bound."""
    import re
    from sparse_rcnn_amd import _lib as L, executor as EX
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "scn_mi355x.h")).read()
    assert re.search(r"SCN_OP_ADD_RELU = %d\b" % EX.OP_ADD_RELU, header) and EX.OP_ADD_RELU == 16
    assert not any(n.startswith("scn_add_relu") for n in L.EXPORTS) and "int scn_add_relu" not in header
    assert "scn_exec_run" in L.EXPORTS and callable(EX.run_add_relu)
    lib = L.load()                                              # (no GPU needed: nothing is launched)
    assert lib.scn_exec_struct_bytes(0) == 64                  # struct sizes stay as they are
