"""Training parts of the network on a frozen rest, the part that needs no GPU: the backward passes a stage derives for what
autograd asks for (`executor.Stage.backward_ops`), and how `SceneStep(train=..., init_state=...)` wires its model, its flat
buffer and its refusals.

The plans are those of tests/golden/make_exec_plans_golden.py: every unit form, fp32 / bf16 storage, batch norm in both
modes, the mask branch's input stage and the stages of a module tree somebody else built -- encoder stages with a stride-1
(level 0) and a stride-2 head, decoder stages.  READS / WRITES below is this test's own account of which fields of an op name
slabs it reads, slabs it writes and gradient regions it writes, written down from the op descriptions in csrc/scn_exec.hip
(`run_op`); nothing of it is imported from the code under test."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_exec_plans_golden as G                              # noqa: E402

from sparse_rcnn_amd import executor as EX                     # noqa: E402
from sparse_rcnn_amd.trainstep import PARTS, SceneStep         # noqa: E402

FIELDS = [n for n, _ in EX.ExecOp._fields_]

# opcode -> (fields read as slabs, fields written as slabs, fields that name a gradient region written)
IO = {
    1: (("x", "r", "m"), ("y",), ()),                  # GEMM_IDENT: y = x W (+ b) (+ r), masked by the sign of m
    2: (("x", "r", "m"), ("y",), ()),                  # CONV_SUBM
    3: (("x", "r", "m"), ("y",), ()),                  # CONV_CHILD
    4: (("x", "m"), ("y",), ()),                       # RULES_CHILD
    5: None,                                           # ROWS2: two forms, below
    6: (("x", "y"), (), ("w", "b")),                   # WGRAD_SUBM: X, dY -> dW, db
    7: (("x", "y", "x1", "y1"), (), ("w", "b")),       # WGRAD2_SUBM: two (X, dY) pairs
    8: (("x", "y"), (), ("w", "b")),                   # WGRAD_DOWN
    9: (("x", "y"), (), ("w", "b")),                   # WGRAD_UP
    10: (("x", "y"), (), ("w", "b")),                  # WGRAD_IDENT
    11: (("x",), (), ("b",)),                          # COLSUM
    12: (("x", "x1"), ("y",), ()),                     # ADD
    13: (("x",), ("y",), ()),                          # CAST
    14: (("x",), ("y",), ()),                          # RELU
    15: (("m", "x1"), ("y",), ()),                     # RELU_BWD: y = x1 masked by the sign of m
    16: (("x", "x1"), ("y",), ()),                     # ADD_RELU
    17: (("x",), ("y",), ()),                          # BN_STATS
    18: (("x", "x1"), ("y",), ()),                     # BN_FWD: mean | var in x1
    19: (("x", "m", "x1"), ("y",), ("b",)),            # BN_BWD: x, dy in m -> dx in y, dgamma | dbeta in region b
}
WGRAD_LIKE = (6, 7, 8, 9, 10, 11)                      # OP_WGRAD* and OP_COLSUM
PARAM_OPS = WGRAD_LIKE + (19,)


def io(op):
    if op.op == 5:                                     # y1 >= 0: one source, two destinations; else two sources, one destination
        names = (("x",), ("y", "y1"), ()) if op.y1 >= 0 else (("x", "x1"), ("y",), ())
    else:
        names = IO[op.op]
    return tuple([getattr(op, f) for f in part if getattr(op, f) >= 0] for part in names)


def fields(op):
    return tuple(getattr(op, f) for f in FIELDS)


@pytest.fixture(scope="module")
def stages():
    out = []
    for gen in (G.unet_cases, G.mask_input_cases, G.tree_cases):
        for name, sts in gen():
            out += [(f"{name}[{k}]", st) for k, st in enumerate(sts)]
    return out


def test_the_stage_kinds_are_covered(stages):
    enc = [st for _, st in stages if st.n_inputs == 1]
    assert any(st.bufs[st.in_ids[0]][0] == st.bufs[st.out_id][0] for st in enc)          # stride-1 head: level 0
    assert any(st.bufs[st.in_ids[0]][0] + 1 == st.bufs[st.out_id][0] for st in enc)      # stride-2 head
    assert any(st.n_inputs == 2 for _, st in stages)                                     # decoder
    assert any(st.bn_layers for _, st in stages) and any(st.bf16 for _, st in stages) and any(not st.bf16 for _, st in stages)
    assert any(op.op == 19 for _, st in stages for op in st.bwd)


def test_everything_needed_is_the_stored_list(stages):
    for name, st in stages:
        ops = st.backward_ops(True, True)
        assert [fields(o) for o in ops] == [fields(o) for o in st.bwd], name
        assert st.backward_ops() == ops
        bp = st.backward_pass(True, True)
        assert bp.arr is st.bwd_arr and bp.ws is st.bwd_ws and bp.specs is st.bwd_specs, name


def _is_subsequence(part, whole):
    it = iter(whole)
    return all(any(p == w for w in it) for p in part)


def test_without_input_gradients(stages):
    shorter = 0
    for name, st in stages:
        ops = st.backward_ops(inputs=False)
        assert ops == st.backward_ops(False, True)
        full = [fields(o) for o in st.bwd]
        kept = [fields(o) for o in ops]
        assert _is_subsequence(kept, full), name
        assert [fields(o) for o in st.bwd if o.op in PARAM_OPS] == [fields(o) for o in ops if o.op in PARAM_OPS], name
        for o in ops:
            _, writes, regions = io(o)
            assert regions or not set(writes) <= set(st.din_ids), (name, fields(o))
        shorter += len(ops) < len(st.bwd)
    # the backward-data op of every stride-2 head and of every deconvolution feeds nothing but the input gradient
    assert shorter >= sum(1 for _, st in stages if st.n_inputs == 2 or st.bufs[st.in_ids[0]][0] != st.bufs[st.out_id][0])


def test_without_parameter_gradients(stages):
    for name, st in stages:
        ops = st.backward_ops(params=False)
        assert ops == st.backward_ops(True, False)
        assert _is_subsequence([fields(o) for o in ops], [fields(o) for o in st.bwd]), name
        assert not [o for o in ops if o.op in WGRAD_LIKE], name
        written = {v for o in ops for v in io(o)[1]}
        assert set(st.din_ids) <= written, name
        assert len(ops) < len(st.bwd), name


def test_nothing_needed_is_nothing_run(stages):
    for name, st in stages:
        assert st.backward_ops(False, False) == [], name
        assert st.backward_ops(inputs=False, params=False) == [], name


@pytest.mark.parametrize("inputs,params", [(True, True), (False, True), (True, False)])
def test_kept_ops_read_what_exists_and_feed_what_is_needed(stages, inputs, params):
    for name, st in stages:
        ops = st.backward_ops(inputs, params)
        forward = set(st.in_ids) | {st.out_id, st.dout_id} | {i for i, b in enumerate(st.bufs) if b[3] == "f"}
        have = set(forward)
        for o in ops:
            reads, writes, _ = io(o)
            assert set(reads) <= have, (name, fields(o))
            have |= set(writes)
        # and the other way round: every kept op writes something a later kept op reads, a needed input gradient or a needed region
        needed = set(st.din_ids) if inputs else set()
        for o in reversed(ops):
            reads, writes, regions = io(o)
            assert (params and regions) or set(writes) & needed, (name, fields(o))
            needed |= set(reads)
        # the stored list and the cached plans stay as they were
        assert len(st.bwd_arr) == len(st.bwd)


def test_the_pass_names_only_what_its_ops_name(stages):
    for name, st in stages:
        for key in ((False, True), (True, False)):
            bp = st.backward_pass(*key)
            named = {v for o in bp.ops for part in io(o)[:2] for v in part}
            assert set(bp.ws) == named & set(st.bwd_ws), name
            assert bp.specs == [(st.bufs[i][0], st.bufs[i][1] * st.bufs[i][2]) for i in bp.ws], name
            assert set(bp.dins) == {v for o in bp.ops for v in io(o)[1]} & set(st.din_ids), name
            assert set(bp.regions) == {v for o in bp.ops for v in io(o)[2]}, name
            assert len(bp.arr) == len(bp.ops) and [fields(o) for o in bp.arr] == [fields(o) for o in bp.ops], name
            assert st.backward_pass(*key) is bp                                          # derived once


# ---- SceneStep(train=..., init_state=...) -----------------------------------------------------------------------------------
# (the mask loss packs its ground truth on the device at construction: the four-loss step is wired in tests/test_gpu_train_parts.py)
CPU = dict(device=torch.device("cpu"), channels=(16, 32), target=500, grid=(32, 32, 16), prefetch=False)
THREE = dict(rpn_loss=True, class_loss=True, segmentation_loss=True)


def _ids(module):
    return {id(p) for p in module.parameters()}


@pytest.fixture(scope="module")
def joint():
    return SceneStep("cfg3-rpn", **THREE, **CPU)


@pytest.mark.parametrize("train", [("mask",), ("rpn", "class"), ("backbone",), ("segmentation", "mask", "rpn", "class"), PARTS])
def test_the_flat_buffer_holds_the_named_parts(joint, train):
    st = SceneStep("cfg3-rpn", train=train, **THREE, **CPU)
    named = set().union(*[_ids(st._part(n)) for n in train])
    assert {id(p) for p in st.flat.params} == named and len(st.flat.params) == len(named)
    for p in st.model.parameters():
        assert p.requires_grad == (id(p) in named)
    assert st.flat.flat.numel() == sum(p.numel() for p in st.flat.params) == st.flat.flat_grad.numel()
    assert st.trainable == tuple(p for p in PARTS if p in train) and st.frozen == tuple(p for p in PARTS if p not in train)
    # same construction as the joint step: the same initial values, frozen or not
    for (k, a), (_, b) in zip(st.model.state_dict().items(), joint.model.state_dict().items()):
        assert torch.equal(a, b), k
    if set(train) == set(PARTS):
        assert len(st.flat.params) == len(joint.flat.params)


def test_train_none_changes_nothing(joint):
    assert joint.train is None and joint.trainable == PARTS and joint.frozen == () and joint.losses_not_computed == ()
    assert all(p.requires_grad for p in joint.model.parameters())
    assert len(joint.flat.params) == sum(1 for _ in joint.model.parameters())
    assert joint.init_missing is None and joint.init_unused is None
    assert "TRAINING IN STAGES" not in joint.describe() and "init_state" not in joint.describe()


def test_which_losses_are_computed():
    def not_computed(train, **kw):
        return SceneStep("cfg3-rpn", train=train, **{**THREE, **kw}, **CPU).losses_not_computed

    assert not_computed(("mask",)) == ("rpn", "class", "segmentation")
    assert not_computed(("rpn", "class")) == ("segmentation",)
    assert not_computed(("backbone",)) == ()
    assert not_computed(("segmentation",)) == ("rpn", "class")
    assert not_computed(("rpn",)) == ("class", "segmentation")
    assert not_computed(("rpn",), dense_class=True) == ("segmentation",)        # the dense class branch reads the RPN's stack
    st = SceneStep("cfg3-rpn", train=("rpn",), **THREE, **CPU)
    assert st.loss_weights() == {"rpn_score": 1.0, "rpn_bbox": 1.0}
    st = SceneStep("cfg3-rpn", train=("class",), loss_weights={"class": 2.0, "rpn_bbox": 0.5}, **THREE, **CPU)
    assert st.combiner.has() == (False, True, False, False) and list(st.loss_weights()) == ["class"]


def test_refusals():
    def build(workload="cfg3-rpn", **kw):
        return SceneStep(workload, **{**CPU, **kw})

    with pytest.raises(ValueError, match="empty"):
        build(train=())
    with pytest.raises(ValueError, match="unknown part"):
        build(train=("mask", "head"))
    with pytest.raises(ValueError, match="tuple"):
        build(train="mask")
    with pytest.raises(ValueError, match="no part 'class'"):
        build(train=("class",), rpn_loss=True)                   # the class branch exists with class_loss=True only
    with pytest.raises(ValueError, match="no part 'segmentation'"):
        build(train=("segmentation",), class_loss=True)
    with pytest.raises(ValueError, match="no part 'rpn'"):
        build("cfg3", train=("rpn",))
    with pytest.raises(ValueError, match="no part 'mask'"):
        build("cfg2", train=("mask",))
    with pytest.raises(ValueError, match="multitask_loss"):
        build(train=("rpn",), rpn_loss=True, multitask_loss=True)
    build("cfg2", train=("backbone",))                           # the one part cfg2 has


def test_describe_names_the_stage():
    d = SceneStep("cfg3-rpn", train=("mask",), **THREE, **CPU).describe()
    assert "train=('mask',)" in d
    assert "trainable parts mask;" in d and "frozen parts backbone, rpn, class, segmentation " in d
    assert "requested losses not computed: rpn, class, segmentation " in d
    d = SceneStep("cfg3-rpn", train=("backbone", "rpn", "class", "segmentation"), **THREE, **CPU).describe()
    assert "frozen parts mask " in d and "requested losses not computed: none " in d


def test_init_state_is_the_ignore_load_rule(joint):
    first = SceneStep("cfg3-rpn", seed=3, **THREE, **CPU)
    with torch.no_grad():                                        # an earlier stage's weights: anything but the seeded initialisation
        for i, p in enumerate(first.model.parameters()):
            p.add_(0.25 + 0.001 * i)
    state = {k: v.clone() for k, v in first.model.state_dict().items() if not k.startswith("class_branch.")}
    state["optimizer.step"] = torch.zeros(())
    st = SceneStep("cfg3-rpn", train=("mask",), init_state=state, **THREE, **CPU)
    own = st.model.state_dict()
    assert st.init_unused == ["optimizer.step"]
    assert st.init_missing == [k for k in own if k.startswith("class_branch.")] and st.init_missing
    for k, v in own.items():
        want = state[k] if k in state else joint.model.state_dict()[k]       # loaded | its own initialisation
        assert torch.equal(v, want), k
    assert "init_state" in st.describe()
    # the flat buffer was built AFTER the load: the trainable parameters are views of it and hold the loaded values
    off = 0
    for p in st.flat.params:
        assert torch.equal(st.flat.flat[off:off + p.numel()].view_as(p), p.data)
        off += p.numel()
    key = next(k for k in state if k.startswith("mask.") and state[k].dim() >= 2)
    bad = dict(state)
    bad[key] = torch.zeros(tuple(state[key].shape) + (2,))
    with pytest.raises(ValueError, match="shape"):
        SceneStep("cfg3-rpn", init_state=bad, **THREE, **CPU)
    full = SceneStep("cfg3-rpn", init_state=first.model.state_dict(), **THREE, **CPU)
    assert full.init_missing == [] and full.init_unused == []
    for (k, a), (_, b) in zip(full.model.state_dict().items(), first.model.state_dict().items()):
        assert torch.equal(a, b), k
