"""-m gpu: training parts of the network on a frozen rest -- `SceneStep(train=..., init_state=...)`, the reference's mask-only
stage (scannet_config/run.py:332,891-893,1376-1427) -- and the stage backward passes cut down to what autograd asks for
(`executor.Stage.backward_pass`).

Every comparison is torch.equal: a frozen step launches the kernels of the joint step with the same arguments or does not
launch them, so no tolerance is involved.  A mask-branch parameter gets its gradient from the mask logits alone: its gradient in
the joint step and in the mask-only step carries the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COMMON = dict(target=10_000, grid=(128, 128, 64), prefetch=False, seed=4, n_gt=4)
FOUR = dict(rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True)


def _step(gpu, **kw):
    from sparse_rcnn_amd.trainstep import SceneStep
    return SceneStep("cfg3-rpn", gpu, **{**COMMON, **kw})


def _forward_backward(st):
    """The forward_backward calls of `SceneStep.step`, without the update."""
    n = st.batches_per_step
    for k in range(n - 1):
        with st.flat.accumulate():
            st.forward_backward(k, zero=(k == 0))
    st.forward_backward(n - 1, zero=(n == 1))
    torch.cuda.synchronize()


def _named(st, *parts):
    return [(f"{part}.{n}", p) for part in parts for n, p in st._part(part).named_parameters()]


@pytest.mark.parametrize("batches_per_step", [1, 2])
@pytest.mark.parametrize("step_group", [True, False], ids=["group", "per-pass"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mask_only_step_has_the_bits_of_the_joint_step(gpu, dtype, step_group, batches_per_step):
    kw = dict(dtype=dtype, step_group=step_group, batches_per_step=batches_per_step, **FOUR)
    joint = _step(gpu, **kw)
    only = _step(gpu, train=("mask",), **kw)
    # wiring of the four-loss step (the mask loss packs its ground truth on the device: not in the CPU file)
    mask_ids = {id(p) for p in only.model.mask.parameters()}
    assert {id(p) for p in only.flat.params} == mask_ids and len(only.flat.params) == len(mask_ids)
    assert all(p.requires_grad == (id(p) in mask_ids) for p in only.model.parameters())
    assert only.losses_not_computed == ("rpn", "class", "segmentation")
    assert "frozen parts backbone, rpn, class, segmentation " in only.describe()
    assert len(joint.flat.params) == sum(1 for _ in joint.model.parameters())

    _forward_backward(joint)
    _forward_backward(only)
    assert only.logits.shape[0] > 0 and torch.equal(only.logits, joint.logits)
    assert torch.equal(only.mask_losses, joint.mask_losses)
    for a, b in zip(only.mask_out[1], joint.mask_out[1]):
        assert torch.equal(a.forward_boxes, b.forward_boxes) and torch.equal(a.gt_association, b.gt_association)
    got, want = _named(only, "mask"), _named(joint, "mask")
    assert len(got) == len(want) > 0
    for (n, p), (_, q) in zip(got, want):
        assert p.grad is not None and q.grad is not None, n
        assert torch.equal(p.grad, q.grad), n
    assert only.rpn_losses is None and only.class_losses is None and only.segmentation_losses is None
    assert joint.rpn_losses is not None and joint.class_losses is not None and joint.segmentation_losses is not None
    assert not only.out.features.requires_grad and joint.out.features.requires_grad
    assert only.fin.grad is None and not only.fin.requires_grad
    for n, p in _named(only, "backbone", "rpn", "class", "segmentation"):
        assert p.grad is None and not p.requires_grad, n
    assert only.n_roi_rows > 0                   # the ground-truth boxes are always appended
    joint.finish()
    only.finish()


def test_frozen_stays_frozen(gpu):
    st = _step(gpu, train=("mask",), optimizer="adam", lr=1e-4, **FOUR)
    before = {n: p.detach().clone() for n, p in st.model.named_parameters()}
    for _ in range(3):
        st.step()
    st.finish()
    torch.cuda.synchronize()
    changed = 0
    for n, p in st.model.named_parameters():
        if n.startswith("mask."):
            changed += not torch.equal(p.detach(), before[n])
        else:
            assert torch.equal(p.detach(), before[n]), n
            assert p.grad is None, n
    assert changed >= 1
    # the optimizer covers the mask branch alone
    assert st.flat.flat.numel() == sum(p.numel() for p in st.model.mask.parameters())


def test_rpn_and_class_on_a_frozen_backbone(gpu):
    st = _step(gpu, train=("rpn", "class"), optimizer="adam", lr=1e-4, **FOUR)
    before = {n: p.detach().clone() for n, p in _named(st, "backbone", "mask", "segmentation")}
    rpn_before = [p.detach().clone() for _, p in _named(st, "rpn", "class")]
    st.step()
    st.finish()
    torch.cuda.synchronize()
    for n, p in _named(st, "backbone", "mask", "segmentation"):
        assert torch.equal(p.detach(), before[n]) and p.grad is None, n
    assert st.rpn_losses is not None and st.class_losses is not None
    assert st.mask_losses is None and st.segmentation_losses is None and st.logits is None     # the mask head did not run
    assert st.losses_not_computed == ("mask", "segmentation")
    assert all(torch.isfinite(t).all() for t in (*st.rpn_losses, st.class_losses))
    assert any(not torch.equal(p.detach(), q) for (_, p), q in zip(_named(st, "rpn", "class"), rpn_before))
    assert not st.out.features.requires_grad


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_backbone_alone_gets_the_joint_steps_gradients(gpu, dtype):
    """Frozen weights, needed input gradients: the RPN and the mask branch pass gradients on and compute none of their own."""
    joint = _step(gpu, dtype=dtype, rpn_loss=True)
    only = _step(gpu, dtype=dtype, rpn_loss=True, train=("backbone",))
    _forward_backward(joint)
    _forward_backward(only)
    assert torch.equal(only.rpn_losses[0], joint.rpn_losses[0]) and torch.equal(only.rpn_losses[1], joint.rpn_losses[1])
    assert torch.equal(only.logits, joint.logits)
    for (n, p), (_, q) in zip(_named(only, "backbone"), _named(joint, "backbone")):
        assert p.grad is not None and torch.equal(p.grad, q.grad), n
    assert torch.equal(only.fin.grad, joint.fin.grad)
    for n, p in _named(only, "rpn", "mask"):
        assert p.grad is None, n
    assert all(q.grad is not None for _, q in _named(joint, "rpn"))
    joint.finish()
    only.finish()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pruned_stage_passes_return_the_full_passes_bits(gpu, dtype):
    from sparse_rcnn_amd import executor as EX
    from sparse_rcnn_amd.synthetic import make_batch
    from sparse_rcnn_amd.unet import Backbone
    coords, feats, size, bs, _ = make_batch(1, (64, 64, 32), 2_000, dup=1.15, seed=9)
    torch.manual_seed(5)
    net = Backbone(7, (16, 32), bf16_blocks="all" if dtype == "bf16" else False).to(gpu)
    plan = net.unet._exec_plan()
    assert plan, "this network must be covered by the executor"
    stages = [s for s in plan["enc"] + plan["dec"] if s is not None]
    gy = None

    def run(inputs, params, scope=False):
        nonlocal gy
        for p in net.parameters():
            p.grad = None
            p.requires_grad_(params)
        fin = feats.to(gpu).requires_grad_(inputs)
        out = net(coords, fin, size, bs)
        assert not EX.LAST_FORWARD["lean"]
        if gy is None:
            gy = torch.randn(out.features.shape, generator=torch.Generator().manual_seed(2)).to(gpu)
        if scope:
            with torch.autograd.set_multithreading_enabled(False), EX.step_weight_gradients():
                out.features.backward(gy)
        else:
            out.features.backward(gy)
        torch.cuda.synchronize()
        ran = dict(EX.LAST_BACKWARD)             # (the last backward pass of the graph: encoder level 0)
        return out.features.detach().clone(), fin.grad, [p.grad for p in net.parameters()], ran

    try:
        out, dfin, grads, ran = run(True, True)
        assert ran["ops"] == ran["of"] == len(stages[0].bwd)
        assert dfin is not None and all(g is not None for g in grads)
        for scope in ((False, True) if dtype == "f32" else (False,)):
            o, d, g, ran = run(False, True, scope)
            assert ran["ops"] == len(stages[0].backward_ops(inputs=False)) < ran["of"]
            assert torch.equal(o, out) and d is None
            for (n, _), a, b in zip(net.named_parameters(), g, grads):
                assert a is not None and torch.equal(a, b), (n, scope)
            if scope:
                assert EX.LAST_STEP_SCOPE["passes"] == len(stages)
        o, d, g, ran = run(True, False)
        assert ran["ops"] == len(stages[0].backward_ops(params=False)) < ran["of"]
        assert torch.equal(o, out) and torch.equal(d, dfin) and all(a is None for a in g)
    finally:
        for p in net.parameters():
            p.requires_grad_(True)


def test_hand_over_between_stages(gpu):
    first = _step(gpu, rpn_loss=True, mask_loss=True, train=("backbone", "rpn"), optimizer="adam", lr=1e-4)
    start = {n: p.detach().clone() for n, p in _named(first, "backbone", "rpn")}
    for _ in range(2):
        first.step()
    first.finish()
    torch.cuda.synchronize()
    trained = {n: p.detach().clone() for n, p in _named(first, "backbone", "rpn")}
    assert any(not torch.equal(trained[n], start[n]) for n in trained)
    second = _step(gpu, rpn_loss=True, mask_loss=True, train=("mask",), init_state=first.model.state_dict(), optimizer="adam",
                   lr=1e-4)
    assert second.init_missing == [] and second.init_unused == []
    for n, p in _named(second, "backbone", "rpn"):
        assert torch.equal(p.detach(), trained[n]), n
    mask_before = [p.detach().clone() for _, p in _named(second, "mask")]
    second.step()
    second.finish()
    torch.cuda.synchronize()
    for n, p in _named(second, "backbone", "rpn"):
        assert torch.equal(p.detach(), trained[n]), n
    assert second.rpn_losses is None and second.mask_losses is not None
    assert any(not torch.equal(p.detach(), q) for (_, p), q in zip(_named(second, "mask"), mask_before))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mask_only_stage_trains(gpu, dtype):
    """The condition of test_gpu_mask_loss.test_scenestep_mask_loss, with no synthetic gradient to neutralise: a frozen
    backbone output has none."""
    st = _step(gpu, dtype=dtype, train=("mask",), optimizer="adam", lr=1e-4, **FOUR)
    losses = []
    for _ in range(20):
        st.step()
        losses.append(float(st.mask_losses.detach().cpu()))
    st.finish()
    print(f"[mask only] cfg3-rpn {dtype}: " + " ".join(f"{v:.4f}" for v in losses))
    assert np.isfinite(losses).all()
    assert losses[-1] < losses[0] and np.mean(losses[-5:]) < losses[0], losses
