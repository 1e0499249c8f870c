"""-m gpu: the order of a scoped fp32 step's end.  The flush of the step scope (csrc/scn_wgrad.hip flush_step) forks when it
holds both grid variants: the job-table copy runs ahead on the library's side stream, then the k_wgrad_group<4> grid and the
weight gradients that launch on their own run there beside k_wgrad_group<2> on the caller's stream, and an event joins them
ahead of the sum launch (SCN_WGRAD_STEP_OVERLAP=0: one stream, the order it had).  Scheduling only -- every kernel keeps its
arguments -- so every comparison here is torch.equal, never a tolerance; a missing join shows up as different bits or as two
runs of one configuration that disagree."""
import ctypes as C

import pytest
import torch

from sparse_rcnn_amd import _lib as L
from sparse_rcnn_amd import executor
from sparse_rcnn_amd import trainstep

pytestmark = pytest.mark.gpu

GRID = (128, 128, 64)
TARGETS = (3_000, 8_000, 20_000)      # the smallest of these at which a cfg2 step launches BOTH grid variants is used
STEPS = 3


def _counts(reset=False):
    out = (C.c_int64 * 4)()
    L.load().scn_wgrad_group_counts(out, 1 if reset else 0)
    return list(out)           # k_wgrad_group<4>, k_wgrad_group<2>, unit launches on their own, sum launches


def _job(gpu, target, **kw):
    args = dict(prefetch=True, seed=1, grad_seed=100, lr=1e-6, target=target, grid=GRID)
    args.update(kw)
    job = trainstep.SceneStep("cfg2", gpu, **args)
    with torch.no_grad():
        g = torch.Generator().manual_seed(21)
        for p in job.model.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return job


def _state(job):
    torch.cuda.synchronize()
    return dict(out=job.out.features.detach().clone(), dfin=job.fin.grad.clone(),
                grads=[(n, None if p.grad is None else p.grad.clone()) for n, p in job.model.named_parameters()],
                params=job.flat.flat.clone())


def _same(a, b):
    assert torch.equal(a["out"], b["out"]), "backbone output"
    assert torch.equal(a["dfin"], b["dfin"]), "input-feature gradient"
    assert len(a["grads"]) == len(b["grads"])
    for (n, x), (_, y) in zip(a["grads"], b["grads"]):
        assert (x is None) == (y is None), n
        if x is not None:
            assert torch.equal(x, y), f"gradient of {n}"
    assert torch.equal(a["params"], b["params"]), "parameters after the update"


def _run(gpu, target, steps=STEPS, **kw):
    """-> the state after `steps` steps of a fresh job, with the launch counts of the last step."""
    job = _job(gpu, target, **kw)
    for k in range(steps):
        if k == steps - 1:
            torch.cuda.synchronize()
            _counts(reset=True)
        executor.LAST_STEP_SCOPE["passes"] = -1
        job.step()
    job.finish()
    st = _state(job)
    st["counts"], st["passes"] = _counts(reset=True), executor.LAST_STEP_SCOPE["passes"]
    return st


@pytest.fixture(scope="module")
def shape(gpu):
    """(target, the state of three steps with every part on): the smallest scene of TARGETS whose step launches one grid of each
    variant -- at least two jobs in each, or flush_step would have launched them on their own -- beside at least one weight
    gradient on its own (the EDGE form of the 7-channel head)."""
    seen = []
    for target in TARGETS:
        st = _run(gpu, target)
        g4, g2, alone, sums = st["counts"]
        seen.append((target, st["counts"]))
        if g4 == 1 and g2 == 1 and alone >= 1:
            return target, st
    raise AssertionError(f"no scene of {TARGETS} launches both k_wgrad_group variants in its step: {seen}")


def test_the_scene_has_both_grids_the_edge_head_and_three_column_sums(gpu, shape):
    target, on = shape
    g4, g2, alone, sums = on["counts"]
    assert (g4, g2) == (1, 1) and alone >= 1 and 1 <= sums <= 2, on["counts"]
    assert on["passes"] == 7
    plan = _job(gpu, target).model.backbone.unet._exec_plan()
    ops = [op.op for st in plan["enc"] + plan["dec"] if st is not None for op in st.bwd]
    assert sum(o == executor.OP_COLSUM for o in ops) == 3
    assert float(on["grads"][0][1].abs().max()) > 0 and bool(torch.isfinite(on["dfin"]).all())


SWITCH = dict(overlap="SCN_WGRAD_STEP_OVERLAP", leaves="SCN_EXEC_HOLD_LEAVES")


@pytest.mark.parametrize("off", ["overlap", "leaves", "both", "step_group", "prefetch"])
def test_each_part_off_gives_the_same_bits(gpu, shape, off):
    target, on = shape
    kw = dict(step_group=False) if off == "step_group" else dict(prefetch=False) if off == "prefetch" else {}
    if off in SWITCH:
        with L.debug_switch(SWITCH[off], 0):
            got = _run(gpu, target, **kw)
    elif off == "both":
        with L.debug_switch(SWITCH["overlap"], 0), L.debug_switch(SWITCH["leaves"], 0):
            got = _run(gpu, target, **kw)
    else:
        got = _run(gpu, target, **kw)
    if off == "step_group":
        assert got["passes"] == -1               # no scope was opened at all: every pass flushed at its own end
    else:
        assert got["passes"] == 7 and got["counts"][:2] == [1, 1]
    _same(on, got)


def test_two_runs_of_one_configuration_agree(gpu, shape):
    """A sum launch that did not wait for the side stream, or an optimizer that ran ahead of it, would read slabs in flight."""
    target, on = shape
    _same(on, _run(gpu, target))


def _net(gpu, ch):
    from sparse_rcnn_amd.unet import Backbone
    torch.manual_seed(3)
    net = Backbone(7, ch).to(gpu)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    assert net.unet._exec_plan(), "this network must be covered by the executor"
    return net


def _scene(target, seed=7):
    from sparse_rcnn_amd.synthetic import make_batch
    coords, feats, size, _, _ = make_batch(1, GRID, target, dup=1.15, seed=seed)
    return coords, feats, size


def _net_step(net, scene, gpu, scope, fail=False):
    """forward + backward of a bare backbone -> ([dX, every parameter gradient], passes held back)."""
    coords, feats, size = scene
    for p in net.parameters():
        p.grad = None
    fin = feats.to(gpu).requires_grad_()
    out = net(coords, fin, size, 1)
    gy = torch.randn(out.features.shape, generator=torch.Generator().manual_seed(11)).to(gpu)
    passes = 0
    with torch.autograd.set_multithreading_enabled(False):          # backward on this thread: the scope is per thread
        if scope:
            with executor.step_weight_gradients():
                out.features.backward(gy)
                if fail:
                    raise ZeroDivisionError
            passes = executor.LAST_STEP_SCOPE["passes"]
        else:
            out.features.backward(gy)
    torch.cuda.synchronize()
    return [fin.grad.clone()] + [p.grad.clone() for p in net.parameters()], passes


@pytest.mark.parametrize("channels", [(32,), (64,)])
def test_a_step_with_one_grid_variant_forks_nothing_and_keeps_its_bits(gpu, shape, channels):
    """A one-level network has one channel width, hence one kind of grouped job: at most one k_wgrad_group variant launches,
    and flush_step forks only when both do."""
    target, _ = shape
    net, scene = _net(gpu, channels), _scene(target)
    ref, _ = _net_step(net, scene, gpu, False)
    torch.cuda.synchronize()
    _counts(reset=True)
    got, passes = _net_step(net, scene, gpu, True)
    g4, g2, alone, sums = _counts(reset=True)
    assert passes == 1
    assert not (g4 and g2), (g4, g2)
    assert g4 + g2 + alone >= 2 and sums >= 1, (g4, g2, alone, sums)
    for x, y in zip(got, ref):
        assert torch.equal(x, y)


def test_after_a_discarded_scope_the_next_step_is_right(gpu, shape):
    target, on = shape
    net, scene = _net(gpu, (32, 64, 128, 256)), _scene(target)
    ref, _ = _net_step(net, scene, gpu, False)
    with pytest.raises(ZeroDivisionError):
        _net_step(net, scene, gpu, True, fail=True)                  # seven passes held back, then dropped
    assert executor.step_scope_passes() is None
    assert L.load().scn_wgrad_step_hold(1) == 0                      # no scope is open on the C side either
    got, passes = _net_step(net, scene, gpu, True)
    assert passes == 7
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
    _same(on, _run(gpu, target))                                     # and a whole step after it has the bits it always had
