"""The reference's bottleneck / main-path-ReLU residual units (unet.residual_block(bottleneck_divisor=, main_path_relu=)) without
a GPU: the float64 restatement the GPU tests compare against (tests/unit_forms_restate.py) meets fixtures the reference's own
dense-mode factory produced; the checkpoint key maps equal the key lists of the reference's FeatureExtractor built with each
switch combination; a reference-format state dict loads completely; the step executor compiles plans for the new units with
the invariants of test_executor_plans_compile_without_a_gpu; the default network's plans are what they were; refusals."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # tests/unit_forms_restate.py
import unit_forms_restate as R                                           # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FORMS = {"bottleneck": dict(bottleneck_divisor=4), "mainpath": dict(main_path_relu=True),
         "both": dict(bottleneck_divisor=4, main_path_relu=True)}
# Both sides are float64 and the fixture's operands are short dyadic numbers (make_unit_forms_golden.py): every sum is exact,
# whatever its order.  1e-12 of the tensor's scale is the bound the comparison is held to; observed: 0.
REL = 1e-12


def _rel(got, ref):
    return float((got.detach() - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


@pytest.mark.parametrize("name", list(FORMS))
def test_restatement_meets_the_references_dense_twin(name):
    g = np.load(os.path.join(GOLD, f"unit_form_{name}.npz"))
    X, P, rules, n, flags, Y, dY, dX, G = R.fixture_unit({k: g[k] for k in g.files})
    assert flags == dict(bottleneck_divisor=FORMS[name].get("bottleneck_divisor", 0),
                         main_path_relu=FORMS[name].get("main_path_relu", False))
    assert X.dtype == torch.float64 and X.shape == (2 * 5 * 4 * 3, 16)
    X = X.clone().requires_grad_()
    P = {k: v.clone().requires_grad_() for k, v in P.items()}
    out = R.unit(X, P, "u", rules, n, **flags)
    assert _rel(out, Y) <= REL
    names = sorted(P)
    grads = torch.autograd.grad(out, [X] + [P[k] for k in names], dY)
    assert _rel(grads[0], dX) <= REL
    for k, got in zip(names, grads[1:]):
        assert got.shape == G[k].shape and _rel(got, G[k]) <= REL, k
    # the masks of its own ReLUs, prescribed through FrozenReLU, give the same function (the form the GPU tests use)
    from oracle import scn_oracle as O
    masks = []
    rec = lambda t: (masks.append(t.detach() > 0), torch.relu(t))[1]
    R.unit(X.detach(), {k: v.detach() for k, v in P.items()}, "u", rules, n, relu=rec, **flags)
    assert len(masks) == R.n_convs(flags["bottleneck_divisor"])              # one ReLU per convolution, whatever the form
    fr = O.FrozenReLU(masks)
    again = R.unit(X, P, "u", rules, n, relu=fr, **flags)
    assert fr.k == len(masks) and torch.equal(again, out)


def _keys():
    with open(os.path.join(GOLD, "unit_forms_keys.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(FORMS))
def test_key_map_equals_the_references_feature_extractor(name):
    from sparse_rcnn_amd.unet import SparseUNet, reference_key_map, unit_conv_indices
    fx = _keys()[name]
    flags = FORMS[name]
    assert {k: bool(v) if k == "main_path_relu" else v for k, v in fx["flags"].items() if v} == flags
    kmap = reference_key_map(len(fx["channels"]), 2, **flags)
    assert sorted(kmap) == sorted(fx["keys"])
    net = SparseUNet(7, fx["channels"], **flags)
    own = net.named_oracle_params()
    assert sorted(own) == sorted(kmap.values())
    for rk, shape in fx["keys"].items():
        assert list(own[kmap[rk]].shape) == shape, rk
    assert sum(p.numel() for p in net.parameters()) == fx["n_params"]
    assert [k for k, _ in R.param_shapes(7, fx["channels"], **flags)] == list(own)
    assert {k: tuple(p.shape) for k, p in own.items()} == dict(R.param_shapes(7, fx["channels"], **flags))
    assert unit_conv_indices() == (1, 3)                      # the default form: dropin_feature_extractor.json


@pytest.mark.parametrize("name", list(FORMS))
def test_reference_state_dict_loads_every_key(name):
    from sparse_rcnn_amd.unet import Backbone, reference_key_map
    fx = _keys()[name]
    g = torch.Generator().manual_seed(3)
    # a checkpoint as the reference writes it: its keys under a prefix, SparseConvNet's grouped layout [fv, 1, nIn, nOut]
    sd = {}
    for k, shape in fx["keys"].items():
        t = torch.randn(shape, generator=g)
        sd["feature_extractor." + k] = t.unsqueeze(1) if len(shape) == 3 else t
    sd["rpn.head.weight"] = torch.zeros(3)                     # somebody else's tensor: neither missing nor unused
    net = Backbone(7, fx["channels"], **FORMS[name])
    missing, unused = net.load_reference_state_dict(sd)
    assert missing == [] and unused == []
    own = net.unet.named_oracle_params()
    for rk, name_ in reference_key_map(len(fx["channels"]), 2, **FORMS[name]).items():
        assert torch.equal(own[name_].detach(), sd["feature_extractor." + rk].reshape(own[name_].shape)), rk
    # a checkpoint of ANOTHER form does not pass for this one
    other = _keys()["mainpath" if name != "mainpath" else "both"]
    with pytest.raises((KeyError, ValueError)):
        net.load_reference_state_dict({"p." + k: torch.zeros(s) for k, s in other["keys"].items()})


def _stages(net):
    plan = net._exec_plan()
    assert plan, "the step executor must cover this network"
    return [s for s in plan["enc"] + plan["dec"] if s is not None]


@pytest.mark.parametrize("bf16", [False, "all"])
@pytest.mark.parametrize("name", list(FORMS))
def test_executor_plans_of_the_new_units(name, bf16):
    """test_executor_plans_compile_without_a_gpu for the new forms, plus: the closing ReLU is an SCN_OP_RELU in place whose
    backward masks by the same slab, slabs of the inner width exist, and the forward-only layout covers every forward slab."""
    from sparse_rcnn_amd import executor as EX
    from sparse_rcnn_amd.unet import SparseUNet
    flags = FORMS[name]
    ch = (32, 64, 96, 128)
    net = SparseUNet(7, ch, bf16_blocks=bf16, **flags)
    stages = _stages(net)
    assert len(stages) == 4 + 3
    seen = []
    main, d = bool(flags.get("main_path_relu")), flags.get("bottleneck_divisor", 0)
    for st in stages:
        for op in st.fwd + st.bwd:
            for field in ("x", "y", "r", "m", "x1", "y1"):
                v = getattr(op, field)
                assert -1 <= v < len(st.bufs), (field, v)
        fwd_ok = {EX.OP_GEMM_IDENT, EX.OP_CONV_SUBM, EX.OP_CONV_CHILD, EX.OP_RULES_CHILD, EX.OP_ROWS2, EX.OP_CAST}
        for op in st.fwd:
            assert -1 <= op.w < len(st.params) and -1 <= op.b < len(st.params)
            assert op.op in (fwd_ok | {EX.OP_RELU} if main else fwd_ok)
        for op in st.bwd:
            if op.op in (EX.OP_WGRAD_SUBM, EX.OP_WGRAD2_SUBM, EX.OP_WGRAD_DOWN, EX.OP_WGRAD_UP, EX.OP_WGRAD_IDENT, EX.OP_COLSUM):
                assert -1 <= op.w < len(st.gregions) and -1 <= op.b < len(st.gregions)
        relus = [op for op in st.fwd if op.op == EX.OP_RELU]
        masks = [op for op in st.bwd if op.op == EX.OP_RELU_BWD]
        assert len(relus) == len(masks) == (2 if main else 0)
        assert all(op.x == op.y for op in relus)                                      # in place
        assert st.bwd_reads_out is main              # the last unit's mask is the stage's output: saved for backward by the node
        assert sorted(op.y for op in relus) == sorted(op.m for op in masks)          # masked by the slab the ReLU wrote
        assert all(op.y not in (op.m, op.x1) and op.y != st.dout_id for op in masks)  # never into the incoming gradient
        # the skip's gradient joins the branch's in one add per unit; neither operand is overwritten
        adds = [op for op in st.bwd if op.op == EX.OP_ADD]
        assert len(adds) == 2 and all(op.y not in (op.x, op.x1) for op in adds)
        if d:
            c = st.bufs[st.out_id][1]
            assert sum(1 for b in st.bufs if b[1] == c // d and b[3] == "f") == 4     # two inner slabs per unit
            assert sum(1 for b in st.bufs if b[1] == c // d and b[3] == "b") == 4
        # every parameter of the stage in exactly one gradient region (freeze() checks it too)
        members = [m for reg in st.gregions for m in reg]
        assert len(members) == len(set(members)) == 2 * len(st.mods)
        # forward-only layout: a slot for every forward slab, no op writes a slot one of its own operands lives in
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
    assert len(convs) == 4 + 3 * 2 + 7 * 2 * R.n_convs(d)


def _digest(net):
    h = hashlib.sha256()
    for st in _stages(net):
        for lst in (st.fwd, st.bwd):
            for op in lst:
                h.update(repr(tuple(getattr(op, f) for f, _ in op._fields_)).encode())
        h.update(repr((st.bufs, [d[:1] + d[1:] for d in st.params], st.gregions, st.in_ids, st.din_ids, st.out_id,
                       st.dout_id, st.lean_classes, st.lean_slot_of)).encode())
    return h.hexdigest()


# The plans the default network compiled BEFORE the unit forms existed (digests taken from that code): every op field, slab,
# parameter slot, gradient region and forward-only slot.
DEFAULT_PLAN_DIGESTS = {
    ((32, 48, 64, 80), False): "05fba194bd24588dcea1698304170f0e4bd83561aa68a714a55cf1a4044b32c3",
    ((32, 48, 64, 80), "all"): "6932da348a6eff40e77deedcd7059c804ff896b636f466d457e113bc2847b606",
}


@pytest.mark.parametrize("key", list(DEFAULT_PLAN_DIGESTS))
def test_default_plans_are_unchanged(key):
    from sparse_rcnn_amd.unet import SparseUNet
    ch, bf16 = key
    torch.manual_seed(0)
    plain = SparseUNet(7, ch, bf16_blocks=bf16)
    assert _digest(plain) == DEFAULT_PLAN_DIGESTS[key]
    explicit = SparseUNet(7, ch, bf16_blocks=bf16, bottleneck_divisor=0, main_path_relu=False)
    assert _digest(explicit) == DEFAULT_PLAN_DIGESTS[key]
    assert repr(explicit) == repr(plain)
    assert list(explicit.state_dict()) == list(plain.state_dict())


def test_refusals():
    from sparse_rcnn_amd.trainstep import SceneStep, SparseStepModel
    from sparse_rcnn_amd.unet import Backbone, SparseUNet, residual_block
    with pytest.raises(ValueError, match="no inner channel"):
        residual_block(3, bottleneck_divisor=4)                                   # C // d == 0
    with pytest.raises(ValueError, match="no inner channel"):
        SparseUNet(7, (4, 8), bottleneck_divisor=8)
    with pytest.raises(ValueError, match="bf16_blocks needs channel counts that are multiples of 8"):
        SparseUNet(7, (16, 32), bf16_blocks="all", bottleneck_divisor=4)          # inner widths 4 and 8
    with pytest.raises(ValueError, match="multiples of 8"):
        SparseStepModel((32, 48), False, "all", bottleneck_divisor=4)             # 48 // 4 = 12
    SparseUNet(7, (32, 64), bf16_blocks="all", bottleneck_divisor=4)              # 8 and 16: fine
    for flags in FORMS.values():
        with pytest.raises(ValueError, match="bf16_blocks=True"):
            SparseUNet(7, (32, 64), bf16_blocks=True, **flags)
    with pytest.raises(ValueError, match="channel-padded"):
        SparseUNet(23, (23, 32), identity_first=True, main_path_relu=True)
    # the switches reach the step's backbone and its description
    m = SparseStepModel((16, 32), False, False, bottleneck_divisor=4, main_path_relu=True)
    assert m.backbone.unet.bottleneck_divisor == 4 and m.backbone.unet.main_path_relu
    assert "C1" in repr(m.backbone.unet.encoder[0][1][0])
    assert Backbone(7, (16, 32)).unet.bottleneck_divisor == 0
    small = dict(device=torch.device("cpu"), channels=(16, 32), target=500, grid=(32, 32, 16), prefetch=False)
    st = SceneStep("cfg2", bottleneck_divisor=4, main_path_relu=True, **small)
    assert "bottleneck_divisor=4" in st.describe() and "main_path_relu=True" in st.describe()
    assert "bottleneck" not in SceneStep("cfg2", **small).describe()
