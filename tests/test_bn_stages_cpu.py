"""Batch-norm networks as step-executor stages (`SparseUNet(batchnorm=True, bn_stages=True)`), without a GPU: the plans compile
for every unit form and input-stage form, every index of every op is in range, every parameter -- gamma and beta of each
batch-norm layer included -- sits in exactly one gradient region of one stage, no ReLU op or fused input ReLU stands where a
batch-norm layer is; the switch is opt-in, the refusals raise, and SCN_EXEC_BN=1 turns it on for a network built without it."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = (16, 32, 48)
FORMS = {"plain": {}, "bottleneck": dict(bottleneck_divisor=4), "mainpath": dict(main_path_relu=True),
         "post": dict(relu_first=False), "input_relu": dict(drop_input_relu=False), "blocks": dict(use_residuals=False),
         "one_unit": dict(num_units=1), "post_input_relu": dict(relu_first=False, drop_input_relu=False)}


def _net(**kw):
    from sparse_rcnn_amd.unet import SparseUNet
    torch.manual_seed(0)
    return SparseUNet(7, CH, batchnorm=True, bn_stages=True, **kw)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", list(FORMS))
def test_plans_of_a_batchnorm_network(name, training):
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd import executor as EX
    from sparse_rcnn_amd import modules as M
    net = _net(**FORMS[name])
    net.train(training)
    plan = net._exec_plan()
    assert plan, "the step executor must cover this network"
    assert len(plan["enc"]) == len(CH) and len(plan["dec"]) == len(CH) - 1          # one stage per level
    stages = plan["enc"] + plan["dec"]
    assert all(isinstance(st, EX.Stage) for st in stages)
    bns = [m for m in net.modules() if isinstance(m, M._BatchNorm)]
    n_units = FORMS[name].get("num_units", 2)
    per_unit = {"plain": 2, "bottleneck": 3, "mainpath": 2, "post": 2, "input_relu": 2, "blocks": 1, "one_unit": 2,
                "post_input_relu": 2}[name]
    # relu_first=False: the decoder's input stages end in an activation, and with drop_input_relu=False the encoder's too;
    # drop_input_relu=False alone: the encoder's lead with one (the decoder's relu_first stage keeps its ReLU module, batch norm
    # or not: unet.py)
    n_stage = {"post": len(CH) - 1, "input_relu": len(CH), "post_input_relu": 2 * len(CH) - 1}.get(name, 0)
    assert len(bns) == (2 * len(CH) - 1) * n_units * per_unit + n_stage
    seen_params, seen_bn = [], []
    for st in stages:
        assert st.bn_training is training
        for op in st.fwd + st.bwd:
            for field in ("x", "y", "r", "m", "x1", "y1"):
                v = getattr(op, field)
                assert -1 <= v < len(st.bufs), (field, v)
            assert 0 <= op.level < len(CH)
        for op in st.fwd:
            assert -1 <= op.w < len(st.params) and -1 <= op.b < len(st.params)
        for op in st.bwd:
            if op.op in (EX.OP_WGRAD_SUBM, EX.OP_WGRAD2_SUBM, EX.OP_WGRAD_DOWN, EX.OP_WGRAD_UP, EX.OP_WGRAD_IDENT, EX.OP_COLSUM):
                assert -1 <= op.w < len(st.gregions) and -1 <= op.b < len(st.gregions)
            elif op.op == EX.OP_BN_BWD:
                assert 0 <= op.w < len(st.params) and 0 <= op.b < len(st.gregions)
            else:
                assert -1 <= op.w < len(st.params)
        # ---- the batch-norm ops: gamma, beta (and in evaluation mode the running buffers) next to each other in the params table
        stage_bn = [(i, m) for i, (m, _) in enumerate(st.mods) if isinstance(m, M._BatchNorm)]
        fwd_bn = [op for op in st.fwd if op.op == EX.OP_BN_FWD]
        bwd_bn = [op for op in st.bwd if op.op == EX.OP_BN_BWD]
        stats = [op for op in st.fwd if op.op == EX.OP_BN_STATS]
        assert len(fwd_bn) == len(bwd_bn) == len(stage_bn)
        assert len(stats) == (len(stage_bn) if training else 0)                    # evaluation plans no statistics op
        assert len(st.bn_layers) == len(stats)
        for op in fwd_bn + bwd_bn:
            mi = st.params[op.w][1]
            m = st.mods[mi][0]
            assert isinstance(m, M._BatchNorm) and op.cin == m.nPlanes
            assert st.params[op.w] == ("w", mi) and st.params[op.w + 1] == ("b", mi)
            assert op.aux == EX._f32_bits(m.eps) and op.c1 == EX._f32_bits(m.leakiness)
            if training:
                assert op.flags & EX.XF_BN_TRAINING and st.bufs[op.x1] == (EX.VEC, 2 * m.nPlanes, 4, "f")
            else:
                assert not op.flags & EX.XF_BN_TRAINING and op.x1 == -1
                assert st.params[op.w + 2] == ("rm", mi) and st.params[op.w + 3] == ("rv", mi)
            assert op.x != op.y and op.y >= 0                                      # a slab of its own, never in place
        for op in bwd_bn:
            mi = st.params[op.w][1]
            assert st.gregions[op.b] == [(mi, "w"), (mi, "b")]                     # dgamma | dbeta
            assert st.bufs[op.y][3] in ("b", "x") and op.m >= 0
        for op in stats:
            assert st.bufs[op.y][0] == EX.VEC and any(f.x1 == op.y and f.x == op.x for f in fwd_bn)
        # both the batch-norm input and its output are forward slabs (kept until the stage's backward) or stage inputs
        for op in fwd_bn:
            assert st.bufs[op.x][3] in ("f", "x") and st.bufs[op.y][3] in ("f", "x")
        # ---- no ReLU where batch norm is: the only fused input ReLU left is the decoder's relu_first ReLU module in front of its
        # deconvolution (unet.py builds M.ReLU there whatever `batchnorm` is); no stand-alone ReLU op anywhere
        for op in st.fwd + st.bwd:
            assert op.op not in (EX.OP_RELU, EX.OP_RELU_BWD, EX.OP_ADD_RELU)
            if op.flags & L.F_RELU_IN:
                assert st in plan["dec"] and not name.startswith("post") and op.op in (EX.OP_RULES_CHILD, EX.OP_WGRAD_UP)
        relu_modules = [m for m in net.modules() if type(m) is M.ReLU]
        assert len(relu_modules) == (0 if name.startswith("post") else len(CH) - 1)
        # ---- every parameter of the stage in exactly one gradient region (freeze() checks it too); no bias beside batch norm
        members = [m for reg in st.gregions for m in reg]
        assert len(members) == len(set(members))
        for i, (m, _) in enumerate(st.mods):
            assert (i, "w") in members and ((i, "b") in members) == (m.bias is not None)
            seen_params += [m.weight] + ([m.bias] if m.bias is not None else [])
        seen_bn += [m for _, m in stage_bn]
        # ---- forward-only layout: a slot for every forward slab, no op writes a slot one of its operands lives in, and the
        # statistics vectors keep theirs (the host reads them after the pass)
        assert len(st.lean_slot_of) == len(st.fwd_ws)
        slot = dict(zip(st.fwd_ws, st.lean_slot_of))
        for op in st.fwd:
            for out in (op.y, op.y1):
                for src in (op.x, op.r, op.m, op.x1):
                    if out in slot and src in slot and out != src:
                        assert slot[out] != slot[src], (op.op, out, src)
        vec_slots = [slot[mv] for _, mv, _ in st.bn_layers]
        assert len(vec_slots) == len(set(vec_slots))
    # every parameter of the NETWORK in exactly one stage
    assert sorted(map(id, seen_params)) == sorted(id(p) for p in net.parameters())
    assert sorted(map(id, seen_bn)) == sorted(map(id, bns))
    for bn in bns:
        assert sum(p is bn.weight for p in seen_params) == 1 and sum(p is bn.bias for p in seen_params) == 1


def test_both_modes_are_cached_apart():
    net = _net()
    a, b = net._exec_plan(training=True), net._exec_plan(training=False)
    assert a is not b and net._exec_plan() is a
    net.eval()
    assert net._exec_plan() is b
    import copy
    twin = copy.deepcopy(net)                                # plans hold ctypes arrays: a copy compiles its own
    assert twin._exec_plan() and twin._exec_plan() is not b


def test_the_switch_is_opt_in():
    from sparse_rcnn_amd.unet import Backbone, SparseUNet
    assert SparseUNet(7, (16, 32), batchnorm=True)._exec_plan() is False
    assert SparseUNet(7, (16, 32), batchnorm=True, bn_stages=False)._exec_plan() is False
    # batchnorm=False: the keyword changes nothing
    a, b = SparseUNet(7, (16, 32)), SparseUNet(7, (16, 32), bn_stages=True)
    assert repr(a) == repr(b) and list(a.state_dict()) == list(b.state_dict())
    pa, pb = a._exec_plan(), b._exec_plan()
    for sa, sb in zip(pa["enc"] + pa["dec"], pb["enc"] + pb["dec"]):
        assert [tuple(getattr(o, f) for f, _ in o._fields_) for o in sa.fwd + sa.bwd] == \
               [tuple(getattr(o, f) for f, _ in o._fields_) for o in sb.fwd + sb.bwd]
        assert not sb.bn_layers and not sb.bn_phys
    # the keyword reaches the network through Backbone and the step's model; the state dict is the same either way
    assert Backbone(7, (16, 32), batchnorm=True, bn_stages=True).unet._exec_plan()
    assert list(Backbone(7, (16, 32), batchnorm=True, bn_stages=True).state_dict()) == \
        list(Backbone(7, (16, 32), batchnorm=True).state_dict())


def test_refusals():
    from sparse_rcnn_amd.trainstep import SparseStepModel
    from sparse_rcnn_amd.unet import SparseUNet
    for storage in (True, "all"):
        with pytest.raises(ValueError, match="bf16_blocks"):
            SparseUNet(7, (16, 32), batchnorm=True, bn_stages=True, bf16_blocks=storage)
    with pytest.raises(ValueError, match="bf16_blocks"):
        SparseStepModel((16, 32), False, "all", batchnorm=True, bn_stages=True)
    with pytest.raises(ValueError, match="batch norm takes no padded slab"):      # the existing refusal, its message kept
        SparseUNet(23, (23, 32), identity_first=True, batchnorm=True, bn_stages=True)
    with pytest.raises(ValueError, match="channel-padded plan"):                   # min_channels: only the skip slab is padded
        SparseUNet(7, (7, 32), identity_first=True, batchnorm=True, bn_stages=True, min_channels=16)
    SparseUNet(7, (7, 32), identity_first=True, batchnorm=True, min_channels=16)   # without the switch: as before


def test_scene_step_takes_the_keyword_and_says_which_path():
    from sparse_rcnn_amd.trainstep import SceneStep
    small = dict(device=torch.device("cpu"), channels=(16, 32), target=500, grid=(32, 32, 16), prefetch=False)
    staged = SceneStep("cfg2-bn", bn_stages=True, **small)
    assert staged.model.backbone.unet.bn_stages and staged.model.backbone.unet._exec_plan()
    assert "step-executor stages" in staged.describe() and "layer-by-layer path" not in staged.describe()
    plain = SceneStep("cfg2-bn", **small)
    assert plain.model.backbone.unet._exec_plan() is False
    assert "layer-by-layer path" in plain.describe() and "step-executor stages" not in plain.describe()
    assert "BatchNorm" not in SceneStep("cfg2", bn_stages=True, **small).describe()


def test_the_developer_switch_turns_the_plan_on():
    code = ("from sparse_rcnn_amd.unet import SparseUNet; from sparse_rcnn_amd import executor as EX; "
            "n = SparseUNet(7, (16, 32), batchnorm=True); p = n._exec_plan(); "
            "print('PLAN', EX.BN_STAGES, bool(p), len(p['enc']) + len(p['dec']) if p else 0)")
    for value, want in (("1", "PLAN True True 3"), ("0", "PLAN False False 0"), (None, "PLAN False False 0")):
        env = {k: v for k, v in os.environ.items() if k != "SCN_EXEC_BN"}
        if value is not None:
            env["SCN_EXEC_BN"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert want in out.stdout, out.stdout
