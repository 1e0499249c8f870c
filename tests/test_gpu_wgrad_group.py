"""-m gpu: grouped weight gradients (csrc/scn_exec.hip + scn_wgrad.hip, k_wgrad_group).  In a backward pass with deferred
sums the executor records the fp32 weight-gradient launches and runs them at the end of the pass as one grid per pass; each
job keeps its plan, its units, its slabs and its fixed-order sum, so grouping on and off (SCN_EXEC_GROUP_WGRAD=0) must give
the same bits for every parameter gradient and the input-feature gradient."""
import pytest
import torch

from sparse_rcnn_amd import _lib as L

pytestmark = pytest.mark.gpu

PLANS = {"bench-150k": ((32, 64, 128, 256), (512, 512, 256), 150_000),
         "bench-small": ((32, 64, 128, 256), (128, 128, 64), 8_000),
         "reference": ((32, 48, 64, 80, 96, 112), (256, 256, 128), 20_000),
         "two-level": ((16, 40), (64, 64, 32), 3_000)}


def _net(gpu, ch, dtype):
    from sparse_rcnn_amd.unet import Backbone
    torch.manual_seed(3)
    net = Backbone(7, ch, bf16_blocks="all" if dtype == "bf16" else False).to(gpu)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    assert net.unet._exec_plan(), "this network must be covered by the executor"
    return net


def _step(net, coords, feats, size, gpu):
    for p in net.parameters():
        p.grad = None
    fin = feats.to(gpu).requires_grad_()
    out = net(coords, fin, size, 1)
    gy = torch.randn(out.features.shape, generator=torch.Generator().manual_seed(11)).to(gpu)
    out.features.backward(gy)
    torch.cuda.synchronize()
    return [fin.grad.clone()] + [p.grad.clone() for p in net.parameters()]


def _scene(grid, target, seed=7):
    from sparse_rcnn_amd.synthetic import make_batch
    coords, feats, size, _, _ = make_batch(1, grid, target, dup=1.15, seed=seed)
    return coords, feats, size


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("plan", list(PLANS))
def test_grouped_weight_gradients_equal_the_launch_by_launch_ones(gpu, dtype, plan):
    ch, grid, target = PLANS[plan]
    coords, feats, size = _scene(grid, target)
    net = _net(gpu, ch, dtype)
    names = ["input features"] + [n for n, _ in net.named_parameters()]
    grouped = _step(net, coords, feats, size, gpu)
    with L.debug_switch("SCN_EXEC_GROUP_WGRAD", 0):
        single = _step(net, coords, feats, size, gpu)
    for n, a, b in zip(names, grouped, single):
        assert torch.equal(a, b), f"gradient of {n}"
    assert float(grouped[1].abs().max()) > 0


def test_grouped_steps_repeat_bit_for_bit(gpu):
    ch, grid, target = PLANS["bench-small"]
    coords, feats, size = _scene(grid, target, seed=9)
    net = _net(gpu, ch, "f32")
    a = _step(net, coords, feats, size, gpu)
    b = _step(net, coords, feats, size, gpu)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("without_deferred_sums", [False, True])
def test_grouping_follows_the_deferred_sums(gpu, without_deferred_sums):
    """Grouping needs the deferred sums (the units' own scratch regions): with SCN_EXEC_DEFER_SUMS=0 every launch is made in
    place, grouping asked for or not -- same bits either way."""
    ch, grid, target = PLANS["two-level"]
    coords, feats, size = _scene(grid, target, seed=5)
    net = _net(gpu, ch, "f32")
    ref = _step(net, coords, feats, size, gpu)
    with L.debug_switch("SCN_EXEC_DEFER_SUMS", 0 if without_deferred_sums else 1):
        for group in (0, 1):
            with L.debug_switch("SCN_EXEC_GROUP_WGRAD", group):
                got = _step(net, coords, feats, size, gpu)
            for x, y in zip(ref, got):
                assert torch.equal(x, y)
