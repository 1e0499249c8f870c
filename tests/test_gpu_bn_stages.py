"""-m gpu: batch-norm networks as step-executor stages (`SparseUNet(batchnorm=True, bn_stages=True)`) against the layer-by-layer
path of the same network, built twice from one seed.  Both paths issue the same entry points with the same arguments in the
same stream order, so every comparison is `torch.equal` -- a condition, not a measured tolerance: output features, encoder
interims, every parameter gradient (gamma and beta included), the input gradient, the running statistics.

Shapes: two samples on a 24x20x16 grid, ~1500 active voxels each with duplicates (test_gpu_parity._cloud), channels (16, 32)
and (8, 16, 24): the smallest that still have a strided level, a decoder level with a two-source 1x1 and tiles with partial
masks."""
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FORMS = {"plain": {}, "bottleneck": dict(bottleneck_divisor=4), "mainpath": dict(main_path_relu=True),
         "post": dict(relu_first=False), "input_relu": dict(drop_input_relu=False), "blocks": dict(use_residuals=False),
         "one_unit": dict(num_units=1), "post_input_relu": dict(relu_first=False, drop_input_relu=False)}
CHANNELS = [(16, 32), (8, 16, 24)]
GRID = (24, 20, 16)


def _cloud(seed, grid=GRID, n=1500, batch=2, dup=200):
    """test_gpu_parity._cloud: `n` distinct voxels per sample, `dup` of them twice, shuffled."""
    rng = np.random.default_rng(seed)
    cs = []
    for b in range(batch):
        lin = rng.choice(grid[0] * grid[1] * grid[2], size=n, replace=False)
        p = np.stack(np.unravel_index(lin, grid), 1)
        p = np.concatenate([p, p[rng.integers(0, n, size=dup)]]) if dup else p
        rng.shuffle(p)
        cs.append(np.concatenate([p, np.full((len(p), 1), b)], 1))
    return torch.from_numpy(np.concatenate(cs).astype(np.int64)), torch.tensor(grid), batch


@pytest.fixture(scope="module")
def scene():
    coords, size, batch = _cloud(5)
    feats = torch.randn(coords.shape[0], 7, generator=torch.Generator().manual_seed(6))
    return coords, feats, size, batch


def _pair(gpu, ch, seed=3, **flags):
    """The same network twice from one seed: as stages, and layer by layer (no keyword).  gamma / beta away from (1, 0)."""
    from sparse_rcnn_amd import modules as M
    from sparse_rcnn_amd.unet import SparseUNet
    nets = []
    for staged in (True, False):
        torch.manual_seed(seed)
        net = SparseUNet(7, ch, batchnorm=True, **(dict(bn_stages=True) if staged else {}), **flags)
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, M._BatchNorm):
                    m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g))
                    m.bias.copy_(0.05 * torch.randn(m.bias.shape, generator=g))
                elif getattr(m, "bias", None) is not None:
                    m.bias.copy_(0.05 * torch.randn(m.bias.shape, generator=g))
        nets.append(net.to(gpu))
    assert nets[0]._exec_plan() and nets[1]._exec_plan() is False
    assert list(nets[0].state_dict()) == list(nets[1].state_dict())
    for a, b in zip(nets[0].state_dict().values(), nets[1].state_dict().values()):
        assert torch.equal(a, b)
    return nets


def _forward(net, gpu, scene):
    import sparse_rcnn_amd as scn
    coords, feats, size, batch = scene
    x = scn.InputLayer(3, size, mode=4)((coords, feats.to(gpu), batch))
    leaf = x.features.detach().requires_grad_()
    y = net(scn.SparseConvNetTensor(leaf, x.metadata, x.spatial_size))
    return leaf, y


def _step(net, gpu, scene, seed=9, scope=False):
    """One training step: forward, then backward from the output AND every encoder interim (the RPN's inputs stay
    differentiable).  -> (output, interims, input gradient, [parameter gradients])"""
    from sparse_rcnn_amd import executor as EX
    for p in net.parameters():
        p.grad = None
    leaf, y = _forward(net, gpu, scene)
    g = torch.Generator().manual_seed(seed)
    roots = [y.features] + [t.features for t in net.interims]
    grads = [torch.randn(t.shape, generator=g).to(gpu) for t in roots]
    if scope:
        with torch.autograd.set_multithreading_enabled(False):      # backward on this thread: the scope is per thread
            with EX.step_weight_gradients():
                torch.autograd.backward(roots, grads)
    else:
        torch.autograd.backward(roots, grads)
    torch.cuda.synchronize()
    return y.features.detach(), [t.features.detach() for t in net.interims], leaf.grad, [p.grad for p in net.parameters()], y


def _nodes(t):
    names, seen, todo = [], set(), [t.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        todo += [g for g, _ in f.next_functions]
    return names


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert bool(torch.isfinite(a).all()), what
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ, max |d| {float((a - b).abs().max()):.3e}"


def _same_step(net_a, net_b, ra, rb, what, nonzero=True):
    _same(ra[0], rb[0], what + " output")
    assert len(ra[1]) == len(rb[1]) == len(net_a.channels)
    for l, (a, b) in enumerate(zip(ra[1], rb[1])):
        _same(a, b, f"{what} interim {l}")
    _same(ra[2], rb[2], what + " input gradient")
    names = [k for k, _ in net_a.named_parameters()]
    assert len(ra[3]) == len(rb[3]) == len(names)
    for k, a, b in zip(names, ra[3], rb[3]):
        assert a is not None and b is not None, k
        _same(a, b, f"{what} grad {k}")
    assert float(ra[0].abs().max()) > 0 and (not nonzero or all(float(g.abs().max()) > 0 for g in ra[3]))


def _same_running(net_a, net_b, what):
    from sparse_rcnn_amd import modules as M
    bns_a = [m for m in net_a.modules() if isinstance(m, M._BatchNorm)]
    bns_b = [m for m in net_b.modules() if isinstance(m, M._BatchNorm)]
    assert len(bns_a) == len(bns_b) > 0
    for i, (a, b) in enumerate(zip(bns_a, bns_b)):
        _same(a.running_mean, b.running_mean, f"{what} running_mean of layer {i}")
        _same(a.running_var, b.running_var, f"{what} running_var of layer {i}")


@pytest.mark.parametrize("ch", CHANNELS, ids=["-".join(map(str, c)) for c in CHANNELS])
@pytest.mark.parametrize("form", list(FORMS))
def test_training_step_is_bit_equal(gpu, scene, form, ch):
    from sparse_rcnn_amd import modules as M
    staged, plain = _pair(gpu, ch, **FORMS[form])
    rs, rp = _step(staged, gpu, scene), _step(plain, gpu, scene)
    _same_step(staged, plain, rs, rp, f"{form} {ch}")
    # graph shape: one StageFunction node per level, no batch-norm node; layer by layer: the other way round
    ns, np_ = _nodes(rs[4].features), _nodes(rp[4].features)
    assert sum(n.startswith("StageFunction") for n in ns) == 2 * len(ch) - 1
    assert not any(n.startswith("BatchNormReLUFunction") for n in ns)
    n_bn = sum(isinstance(m, M._BatchNorm) for m in plain.modules())
    assert sum(n.startswith("BatchNormReLUFunction") for n in np_) == n_bn and not any(n.startswith("StageFunction") for n in np_)
    _same_running(staged, plain, f"{form} {ch} after one step:")
    # the running buffers moved: zeros -> 0.1 * mean, ones -> 0.9 + 0.1 * f * var
    assert any(float(m.running_mean.abs().max()) > 0 for m in staged.modules() if isinstance(m, M._BatchNorm))


@pytest.mark.parametrize("ch", CHANNELS, ids=["-".join(map(str, c)) for c in CHANNELS])
def test_running_statistics_after_two_steps(gpu, scene, ch):
    staged, plain = _pair(gpu, ch)
    coords2, size, batch = _cloud(8)
    scene2 = (coords2, torch.randn(coords2.shape[0], 7, generator=torch.Generator().manual_seed(12)), size, batch)
    for k, sc in enumerate((scene, scene2)):
        rs, rp = _step(staged, gpu, sc, seed=20 + k), _step(plain, gpu, sc, seed=20 + k)
        _same_step(staged, plain, rs, rp, f"step {k}")
    _same_running(staged, plain, "after two steps:")


@pytest.mark.parametrize("ch", CHANNELS, ids=["-".join(map(str, c)) for c in CHANNELS])
def test_eval_mode_reads_the_running_buffers_and_writes_none(gpu, scene, ch):
    from sparse_rcnn_amd import executor as EX
    from sparse_rcnn_amd import modules as M
    staged, plain = _pair(gpu, ch)
    _step(staged, gpu, scene), _step(plain, gpu, scene)              # running buffers away from (0, 1)
    staged.eval(), plain.eval()
    before = [t.clone() for m in staged.modules() if isinstance(m, M._BatchNorm) for t in (m.running_mean, m.running_var)]
    rs, rp = _step(staged, gpu, scene), _step(plain, gpu, scene)     # a backward through the evaluation-mode statistics too
    _same_step(staged, plain, rs, rp, "eval")
    assert sum(n.startswith("StageFunction") for n in _nodes(rs[4].features)) == 2 * len(ch) - 1
    after = [t for m in staged.modules() if isinstance(m, M._BatchNorm) for t in (m.running_mean, m.running_var)]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    _same_running(staged, plain, "eval:")
    with torch.no_grad():                                            # forward-only layout: nothing kept, same bits
        _, yn = _forward(staged, gpu, scene)
        assert EX.LAST_FORWARD["lean"] and yn.features.grad_fn is None
        _, yp = _forward(plain, gpu, scene)
    _same(yn.features, rs[0], "no_grad forward against the evaluation forward")
    _same(yn.features, yp.features, "no_grad forward, staged against layer by layer")
    for a, b in zip(staged.interims, rs[1]):
        _same(a.features, b, "no_grad interim")
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    # training mode under no_grad: the forward-only layout still hands the statistics back
    staged.train(), plain.train()
    with torch.no_grad():
        _, yn = _forward(staged, gpu, scene)
        assert EX.LAST_FORWARD["lean"]
        _, yp = _forward(plain, gpu, scene)
    _same(yn.features, yp.features, "training-mode no_grad forward")
    _same_running(staged, plain, "training-mode no_grad forward:")
    assert not all(torch.equal(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("form", ["plain", "bottleneck"])
def test_step_weight_gradients_scope(gpu, scene, form):
    from sparse_rcnn_amd import executor as EX
    staged, plain = _pair(gpu, (8, 16, 24), **FORMS[form])
    rs = _step(staged, gpu, scene, scope=True)
    assert EX.LAST_STEP_SCOPE["passes"] == 5 and EX.LAST_STEP_SCOPE["delivered"] > 0      # every level was held back
    rp = _step(plain, gpu, scene)
    _same_step(staged, plain, rs, rp, f"step scope {form}")
    again = _step(staged, gpu, scene)                                 # and without the block
    _same_step(staged, staged, rs, again, f"step scope {form} against no scope")


def test_one_row_level_and_an_empty_sample(gpu):
    """Level 2 holds ONE row (every voxel inside one 4^3 cell: n = 1, where the unbiased factor is skipped and the biased
    variance is 0) and the second sample of the batch has no voxel at all (its coarsest level is empty)."""
    rng = np.random.default_rng(2)
    lin = rng.choice(64, size=40, replace=False)
    p = np.stack(np.unravel_index(lin, (4, 4, 4)), 1) + np.array([8, 4, 12])
    coords = torch.from_numpy(np.concatenate([p, np.zeros((len(p), 1), np.int64)], 1).astype(np.int64))
    feats = torch.randn(coords.shape[0], 7, generator=torch.Generator().manual_seed(1))
    sc = (coords, feats, torch.tensor(GRID), 2)
    staged, plain = _pair(gpu, (8, 16, 24))
    rs, rp = _step(staged, gpu, sc), _step(plain, gpu, sc)
    assert [t.shape[0] for t in rs[1]] == [40, rs[1][1].shape[0], 1] and 1 <= rs[1][1].shape[0] <= 8
    assert sum(n.startswith("StageFunction") for n in _nodes(rs[4].features)) == 5
    # (a one-row level normalises to beta exactly: the gradients of what feeds it are zero, on both paths)
    _same_step(staged, plain, rs, rp, "one-row level", nonzero=False)
    assert sum(float(g.abs().max()) > 0 for g in rs[3]) >= len(rs[3]) // 2
    _same_running(staged, plain, "one-row level:")


def test_syncbn_with_a_process_group_falls_back(gpu, scene):
    import torch.distributed as dist
    from sparse_rcnn_amd import modules as M
    staged, plain = _pair(gpu, (16, 32))
    assert not dist.is_initialized()
    with tempfile.TemporaryDirectory() as d:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "store"), rank=0, world_size=1)
        M._BatchNorm.SYNC = True
        try:
            rs, rp = _step(staged, gpu, scene), _step(plain, gpu, scene)
        finally:
            M._BatchNorm.SYNC = False
            dist.destroy_process_group()
    names = _nodes(rs[4].features)
    assert not any(n.startswith("StageFunction") for n in names) and any(n.startswith("BatchNormReLUFunction") for n in names)
    _same_step(staged, plain, rs, rp, "SyncBN fallback")
    _same_running(staged, plain, "SyncBN fallback:")
    rs = _step(staged, gpu, scene)                                    # the switch off again: stages again
    assert sum(n.startswith("StageFunction") for n in _nodes(rs[4].features)) == 3


def test_recording_activation_masks_falls_back(gpu, scene):
    """functional.RELU_RECORD (the parity tests' frozen masks): a staged batch-norm network runs layer by layer while it is on
    (DESIGN section 4.19), so the recorded masks are the layer-by-layer path's."""
    from sparse_rcnn_amd import functional as F
    from sparse_rcnn_amd import modules as M
    staged, plain = _pair(gpu, (16, 32))
    got = []
    for net in (staged, plain):
        F.RELU_RECORD = []
        try:
            _, y = _forward(net, gpu, scene)
            got.append((y.features.detach(), F.RELU_RECORD))
        finally:
            F.RELU_RECORD = None
    _same(got[0][0], got[1][0], "recorded forward")
    n_bn = sum(isinstance(m, M._BatchNorm) for m in staged.modules())
    assert len(got[0][1]) == len(got[1][1]) == n_bn + 1              # + the decoder's ReLU in front of its deconvolution
    assert all(torch.equal(a, b) for a, b in zip(got[0][1], got[1][1]))


def test_cfg2_bn_step_at_150k(gpu):
    """`SceneStep("cfg2-bn", bn_stages=True)` against the same step without the flag on the workload's 150 000 voxels: the
    output the step's loss direction is applied to, every gradient and the running statistics after one step."""
    from sparse_rcnn_amd import modules as M
    from sparse_rcnn_amd.trainstep import SceneStep
    jobs = [SceneStep("cfg2-bn", gpu, prefetch=False, seed=1, grad_seed=100, lr=0.0, **kw) for kw in (dict(bn_stages=True), {})]
    assert jobs[0].model.backbone.unet._exec_plan() and jobs[1].model.backbone.unet._exec_plan() is False
    assert "step-executor stages" in jobs[0].describe() and "layer-by-layer path" in jobs[1].describe()
    for job in jobs:
        job.forward_backward()
    torch.cuda.synchronize()
    a, b = jobs
    assert a.out.features.shape == (150_000, 32)
    assert sum(n.startswith("StageFunction") for n in _nodes(a.out.features)) == 7
    assert not any(n.startswith("BatchNormReLUFunction") for n in _nodes(a.out.features))
    _same(a.out.features.detach(), b.out.features.detach(), "cfg2-bn output")
    _same(a._gys[0], b._gys[0], "cfg2-bn upstream gradient")
    _same(a.fin.grad, b.fin.grad, "cfg2-bn input gradient")
    pa, pb = dict(a.model.named_parameters()), dict(b.model.named_parameters())
    assert list(pa) == list(pb)
    for k in pa:
        assert pa[k].grad is not None and pb[k].grad is not None, k
        _same(pa[k].grad, pb[k].grad, "cfg2-bn grad " + k)
    n_bn = sum(isinstance(m, M._BatchNorm) for m in a.model.modules())
    assert n_bn == 28
    _same_running(a.model, b.model, "cfg2-bn")
