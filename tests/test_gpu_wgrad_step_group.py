"""-m gpu: the step scope of the weight gradients (executor.step_weight_gradients; csrc/scn_wgrad.hip scn_wgrad_step_begin /
_hold / _flush).  Inside the scope the backward passes of the compiled fp32 stages hold their weight-gradient launches and
unit sums back, and the scope's exit runs them as one k_wgrad_group grid per kernel variant and one sum launch.  Every job
keeps its plan, its units, its slabs, its instantiation and its fixed-order sum, so the scope on and off
(SCN_EXEC_GROUP_STEP=0: every pass flushes at its own end) must give the same bits: outputs, input-feature gradient, every
parameter gradient and the updated parameters are compared with torch.equal, never with a tolerance."""
import ctypes as C

import pytest
import torch

from sparse_rcnn_amd import _lib as L
from sparse_rcnn_amd import executor

pytestmark = pytest.mark.gpu

SMALL = dict(target=8_000, grid=(128, 128, 64))


def _counts(reset=False):
    out = (C.c_int64 * 4)()
    L.load().scn_wgrad_group_counts(out, 1 if reset else 0)
    return list(out)           # k_wgrad_group<4>, k_wgrad_group<2>, unit launches on their own, sum launches


def _job(gpu, workload="cfg2", **kw):
    from sparse_rcnn_amd.trainstep import SceneStep
    args = dict(prefetch=False, seed=1, grad_seed=100)
    args.update(kw)
    job = SceneStep(workload, gpu, **args)
    with torch.no_grad():
        g = torch.Generator().manual_seed(21)
        for p in job.model.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return job


def _state(job):
    torch.cuda.synchronize()
    return dict(out=job.out.features.detach().clone(), logits=None if job.logits is None else job.logits.detach().clone(),
                dfin=job.fin.grad.clone(),
                grads=[(n, None if p.grad is None else p.grad.clone()) for n, p in job.model.named_parameters()],
                params=job.flat.flat.clone())


def _same(a, b):
    assert torch.equal(a["out"], b["out"]), "output"
    assert (a["logits"] is None) == (b["logits"] is None)
    if a["logits"] is not None:
        assert torch.equal(a["logits"], b["logits"]), "mask logits"
    assert torch.equal(a["dfin"], b["dfin"]), "input-feature gradient"
    assert len(a["grads"]) == len(b["grads"])
    for (n, x), (_, y) in zip(a["grads"], b["grads"]):
        assert (x is None) == (y is None), n
        if x is not None:
            assert torch.equal(x, y), f"gradient of {n}"
    assert torch.equal(a["params"], b["params"]), "parameters after the update"


def _step(job):
    executor.LAST_STEP_SCOPE["passes"] = executor.LAST_STEP_SCOPE["delivered"] = -1
    job.step()
    job.finish()
    st = _state(job)
    st["passes"], st["delivered"] = executor.LAST_STEP_SCOPE["passes"], executor.LAST_STEP_SCOPE["delivered"]
    return st


def _on_and_off(gpu, workload, **kw):
    on = _step(_job(gpu, workload, **kw))
    with L.debug_switch("SCN_EXEC_GROUP_STEP", 0):
        off = _step(_job(gpu, workload, **kw))
    assert off["passes"] == 0 and off["delivered"] == 0
    _same(on, off)
    return on, off


# ---- (a) same bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cfg2-small", "cfg2-150k", "cfg3-small"])
def test_step_scope_gives_the_bits_of_the_per_pass_flush(gpu, case):
    if case == "cfg2-small":
        on, _ = _on_and_off(gpu, "cfg2", **SMALL)
        assert on["passes"] == 7                                   # one compiled stage per U-Net level stage, all eligible
    elif case == "cfg2-150k":
        on, _ = _on_and_off(gpu, "cfg2")
        assert on["out"].shape[0] == 150_000 and on["passes"] == 7
    else:
        on, _ = _on_and_off(gpu, "cfg3", n_boxes=8, seed=5, grad_seed=9, target=10_000, grid=(128, 128, 64))
        assert on["logits"].shape[0] > 0 and on["passes"] >= 7     # the backbone's stages at least
    assert on["delivered"] > 0
    assert float(on["grads"][0][1].abs().max()) > 0


# ---- (b) repeatable -------------------------------------------------------------------------------------------------------
def test_two_steps_with_the_scope_repeat_bit_for_bit(gpu):
    """lr = 0: the second step sees the parameters of the first, so every output and gradient must repeat."""
    job = _job(gpu, "cfg2", lr=0.0, **SMALL)
    a = _step(job)
    b = _step(job)
    assert a["passes"] == b["passes"] == 7
    _same(a, b)


# ---- (c) one grid per variant ---------------------------------------------------------------------------------------------
def test_one_grouped_launch_per_variant_and_step(gpu):
    """The cfg2 fp32 step has 7 backward passes with 3 (encoder) or 5 (decoder) weight-gradient ops each -- at most six, so a
    pass's flush is one grouped launch and one sum launch: 7 and 7 per step with SCN_EXEC_GROUP_STEP=0.  With the scope:
    at most one launch of each k_wgrad_group variant and at most two sum launches."""
    job = _job(gpu, "cfg2", **SMALL)
    _step(job)                                   # (first step: nothing to learn from its counts)
    _counts(reset=True)
    st = _step(job)
    g4, g2, alone, sums = _counts(reset=True)
    assert st["passes"] == 7
    assert g4 <= 1 and g2 <= 1 and g4 + g2 >= 1, (g4, g2)
    assert 1 <= sums <= 2, sums
    with L.debug_switch("SCN_EXEC_GROUP_STEP", 0):
        _step(job)
        h4, h2, alone0, sums0 = _counts(reset=True)
    assert h4 + h2 == 7 and sums0 == 7, (h4, h2, sums0)
    assert alone0 >= alone - 2                   # (a variant with a single job in the step launches on its own)


# ---- (d) fallbacks --------------------------------------------------------------------------------------------------------
def _net(gpu, ch=(32, 64, 128, 256)):
    from sparse_rcnn_amd.unet import Backbone
    torch.manual_seed(3)
    net = Backbone(7, ch).to(gpu)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    assert net.unet._exec_plan(), "this network must be covered by the executor"
    return net


def _scene(grid=(128, 128, 64), target=8_000, seed=7):
    from sparse_rcnn_amd.synthetic import make_batch
    coords, feats, size, _, _ = make_batch(1, grid, target, dup=1.15, seed=seed)
    return coords, feats, size


def _net_step(net, scene, gpu, scope, prepare=None, retain=False, graph=None):
    """forward + backward of a bare backbone; -> ([dX, every parameter gradient], passes held back, (out, fin, gy))."""
    coords, feats, size = scene
    for p in net.parameters():
        p.grad = None
    if prepare is not None:
        prepare(net)
    if graph is None:
        fin = feats.to(gpu).requires_grad_()
        out = net(coords, fin, size, 1)
        gy = torch.randn(out.features.shape, generator=torch.Generator().manual_seed(11)).to(gpu)
    else:
        out, fin, gy = graph
        fin.grad = None
    passes = 0
    with torch.autograd.set_multithreading_enabled(False):          # backward on this thread: the scope is per thread
        if scope:
            with executor.step_weight_gradients():
                out.features.backward(gy, retain_graph=retain)
            passes = executor.LAST_STEP_SCOPE["passes"]
        else:
            out.features.backward(gy, retain_graph=retain)
    torch.cuda.synchronize()
    return [fin.grad.clone()] + [p.grad.clone() for p in net.parameters()], passes, (out, fin, gy)


def test_a_parameter_with_a_gradient_keeps_its_stage_in_place(gpu):
    net, scene = _net(gpu), _scene()
    first = next(net.parameters())

    def prepare(n):
        p = next(n.parameters())
        p.grad = torch.full_like(p, 0.25)
    got, passes, _ = _net_step(net, scene, gpu, True, prepare)
    ref, _, _ = _net_step(net, scene, gpu, False, prepare)
    assert passes == 6                                               # the stage that owns `first` ran in place
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
    plain, _, _ = _net_step(net, scene, gpu, False)
    k = 1 + [id(p) for p in net.parameters()].index(id(first))
    assert torch.equal(got[k], plain[k] + 0.25)                      # autograd accumulated into the existing .grad


def test_a_parameter_with_a_hook_keeps_its_stage_in_place(gpu):
    net, scene = _net(gpu), _scene()
    calls = []
    h = next(net.parameters()).register_hook(lambda g: calls.append(1) or g)
    try:
        got, passes, _ = _net_step(net, scene, gpu, True)
        assert passes == 6 and len(calls) == 1                       # the hook saw its gradient during backward
        ref, _, _ = _net_step(net, scene, gpu, False)
    finally:
        h.remove()
    for x, y in zip(got, ref):
        assert torch.equal(x, y)


def test_a_channel_padded_stage_runs_in_place(gpu):
    """cfg3: level 0 of the mask branch's internal U-Net runs on slabs padded from 23 to 24 columns; its stage sees padded
    views of the parameters and autograd carries their gradients back through the pad, so it cannot be delivered late."""
    kw = dict(n_boxes=8, seed=5, grad_seed=9, target=10_000, grid=(128, 128, 64))
    job = _job(gpu, "cfg3", **kw)
    assert any(getattr(m, "pad_out_to", None) for m in job.model.modules())
    on = _step(job)
    n_stage, seen, todo = 0, set(), [job.out.features.grad_fn, job.logits.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        n_stage += type(f).__name__.startswith("StageFunction")
        todo += [g for g, _ in f.next_functions]
    assert 7 <= on["passes"] < n_stage, (on["passes"], n_stage)
    with L.debug_switch("SCN_EXEC_GROUP_STEP", 0):
        off = _step(_job(gpu, "cfg3", **kw))
    _same(on, off)


def test_bf16_storage_runs_in_place(gpu):
    on, _ = _on_and_off(gpu, "cfg2", dtype="bf16", **SMALL)
    assert on["passes"] == 0 and on["delivered"] == 0


# ---- (e) gradient accumulation --------------------------------------------------------------------------------------------
def test_gradient_accumulation_equals_the_per_pass_flush(gpu):
    """SceneStep opens no scope under `FlatParams.accumulate()` and the last micro-batch finds `.grad` set: every pass of a
    batches_per_step = 2 step runs in place (pinned here), with the bits of the switch at 0."""
    on, _ = _on_and_off(gpu, "cfg2", batches_per_step=2, **SMALL)
    assert on["passes"] == 0 and on["delivered"] == 0


def _twice(net, scene, gpu, scope, two_backwards):
    """One network applied to two inputs in one graph (or backpropagated by two calls inside one block): every parameter gets
    two gradients.  -> [dX1, dX2, every parameter gradient], passes held back"""
    coords, feats, size = scene
    for p in net.parameters():
        p.grad = None
    f1 = feats.to(gpu).requires_grad_()
    f2 = (feats * 0.5).to(gpu).requires_grad_()
    o1, o2 = net(coords, f1, size, 1), net(coords, f2, size, 1)
    gy = torch.randn(o1.features.shape, generator=torch.Generator().manual_seed(11)).to(gpu)
    import contextlib
    passes = 0
    with torch.autograd.set_multithreading_enabled(False):
        with (executor.step_weight_gradients() if scope else contextlib.nullcontext()):
            if two_backwards:
                o1.features.backward(gy)
                o2.features.backward(gy * 2)
            else:
                torch.autograd.backward([o1.features, o2.features], [gy, gy * 2])
        if scope:
            passes = executor.LAST_STEP_SCOPE["passes"]
    torch.cuda.synchronize()
    return [f1.grad.clone(), f2.grad.clone()] + [p.grad.clone() for p in net.parameters()], passes


@pytest.mark.parametrize("two_backwards", [False, True])
def test_a_parameter_used_by_two_passes_of_one_block_gets_the_sum(gpu, two_backwards):
    """Held back once, in place the second time, added at exit: the sum of two terms autograd forms without the block (fp32
    addition of two terms does not depend on their order, so torch.equal is the bound)."""
    net, scene = _net(gpu), _scene()
    got, passes = _twice(net, scene, gpu, True, two_backwards)
    ref, _ = _twice(net, scene, gpu, False, two_backwards)
    assert passes == 7                                               # each of the 7 stages is held back for ONE of its two passes
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
    coords, feats, size = scene                                      # and it IS a sum: not the gradient of one application
    one, _, _ = _net_step(net, scene, gpu, False)
    assert not torch.equal(got[2], one[1])


def test_some_stages_held_while_others_accumulate(gpu):
    """Gradient accumulation by hand: the encoder's parameters carry a gradient from an earlier micro-batch, the decoder's
    were dropped -- the decoder stages are held back, the encoder stages accumulate in place."""
    net, scene = _net(gpu), _scene()
    first, _, _ = _net_step(net, scene, gpu, False)
    enc = {id(p) for p in net.unet.encoder.parameters()}
    params = list(net.parameters())
    assert 0 < len(enc) < len(params)

    def prepare(n):
        for p, g in zip(n.parameters(), first[1:]):
            p.grad = g.clone() if id(p) in enc else None
    got, passes, _ = _net_step(net, scene, gpu, True, prepare)
    ref, _, _ = _net_step(net, scene, gpu, False, prepare)
    assert passes == 3                                               # the three decoder stages of a four-level U-Net
    for x, y in zip(got, ref):
        assert torch.equal(x, y)


def test_scene_step_without_the_scope(gpu):
    on = _step(_job(gpu, "cfg2", **SMALL))
    off = _step(_job(gpu, "cfg2", step_group=False, **SMALL))
    assert on["passes"] == 7 and off["passes"] == -1                 # (-1: no scope was opened at all)
    _same(on, off)


# ---- (f) failure and reuse ------------------------------------------------------------------------------------------------
def test_an_exception_inside_the_scope_leaves_no_recorder_open(gpu):
    net, scene = _net(gpu), _scene()
    ref, _, _ = _net_step(net, scene, gpu, False)
    coords, feats, size = scene
    for p in net.parameters():
        p.grad = None
    fin = feats.to(gpu).requires_grad_()
    out = net(coords, fin, size, 1)
    gy = torch.ones_like(out.features)
    with pytest.raises(ZeroDivisionError):
        with torch.autograd.set_multithreading_enabled(False), executor.step_weight_gradients():
            out.features.backward(gy)            # seven passes are held back ...
            assert executor.step_scope_passes() == 7
            1 / 0                                # ... and dropped
    assert executor.step_scope_passes() is None
    assert L.load().scn_wgrad_step_hold(1) == 0                      # no scope is open on the C side either
    with pytest.raises(RuntimeError):
        with executor.step_weight_gradients():
            with executor.step_weight_gradients():
                pass
    assert executor.step_scope_passes() is None
    got, passes, _ = _net_step(net, scene, gpu, True)                # the next step is correct
    assert passes == 7
    for x, y in zip(got, ref):
        assert torch.equal(x, y)


def test_a_second_backward_over_a_retained_graph_in_a_new_scope(gpu):
    net, scene = _net(gpu), _scene()
    ref, _, _ = _net_step(net, scene, gpu, False)
    a, pa, graph = _net_step(net, scene, gpu, True, retain=True)
    b, pb, _ = _net_step(net, scene, gpu, True, graph=graph)
    assert pa == pb == 7
    for x, y, z in zip(ref, a, b):
        assert torch.equal(x, y) and torch.equal(x, z)
