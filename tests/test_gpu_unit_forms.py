"""-m gpu: the reference's bottleneck / main-path-ReLU residual units (unet.residual_block(bottleneck_divisor=, main_path_relu=))
on the device -- single units against the float64 restatement (tests/unit_forms_restate.py, itself pinned against the
reference's dense-mode factory in tests/test_unit_forms_cpu.py), a two-level SparseUNet through the step executor against the
layer-by-layer path (all bits), forward-only against the training forward (all bits), the fall-back without levels, one
SceneStep per form against the restatement, and a reference-format checkpoint.

Bounds: fp32 forward features within 1e-4 of the output's scale against the restatement's OWN ReLU
decisions; gradients with the ReLU masks the HIP forward recorded prescribed to the restatement (FrozenReLU) within 2e-5
relative L2 in fp32 and 2e-2 in bf16 storage, there against the restatement with the same storage roundings; the bf16
forward against that restatement within the project's bf16 forward bound (2^-6 of the scale, 1e-2 relative L2)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # tests/unit_forms_restate.py
import unit_forms_restate as R                                           # noqa: E402
from oracle import scn_oracle as O                                       # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = {"bottleneck": dict(bottleneck_divisor=4), "mainpath": dict(main_path_relu=True),
         "both": dict(bottleneck_divisor=4, main_path_relu=True)}
FEAT_TOL, L2_F32, L2_BF16 = 1e-4, 2e-5, 2e-2
BF16_FWD_SCALE, BF16_FWD_L2 = 2.0 ** -6, 1e-2


class _Round(torch.autograd.Function):
    """bf16 storage of a slab at the restatement's own dtype (O.bf16_storage returns fp32), straight-through backward."""

    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def _q(t):
    return _Round.apply(t)


class _masks:
    def __enter__(self):
        from sparse_rcnn_amd import functional as F
        F.RELU_RECORD = []
        return F.RELU_RECORD

    def __exit__(self, *exc):
        from sparse_rcnn_amd import functional as F
        F.RELU_RECORD = None
        return False


def _scale_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def _l2(got, ref):
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().double().reshape(-1)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def _check(what, got, ref, bound, measure=_l2):
    e = measure(got, ref)
    print(f"[unit-forms] {what}: {e:.3e} (bound {bound:.1e})")
    assert bool(torch.isfinite(got).all()) and e <= bound, (what, e, bound)


def _n_stage_nodes(t):
    n, seen, todo = 0, set(), [t.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        n += type(f).__name__.startswith("StageFunction")
        todo += [g for g, _ in f.next_functions]
    return n


def _f64(P):
    return {k: v.detach().cpu().double().clone().requires_grad_() for k, v in P.items()}


# ------------------------------------------------------------------------------------------------------------ single units
@pytest.fixture(scope="module")
def cloud():
    """~300 active sites per sample in a 12^3 grid, two samples, unique sites (rows = input order) + their 3^3 rules."""
    rng = np.random.default_rng(11)
    cs = []
    for b in range(2):
        lin = rng.choice(12 ** 3, size=300 + 7 * b, replace=False)
        p = np.stack(np.unravel_index(lin, (12, 12, 12)), 1)
        cs.append(np.concatenate([p, np.full((len(p), 1), b)], 1))
    coords = np.concatenate(cs).astype(np.int64)
    return coords, O.subm_rulebook(coords, 3)[1]


UNIT_WIDTHS = [("f32", 16, 4), ("f32", 36, 3), ("bf16", 32, 4), ("bf16", 96, 4)]      # inner widths 4, 12, 8, 24


@pytest.mark.parametrize("dtype,C,d", UNIT_WIDTHS, ids=[f"{t}-C{c}-d{d}" for t, c, d in UNIT_WIDTHS])
@pytest.mark.parametrize("form", list(FORMS))
def test_single_unit_against_the_restatement(gpu, cloud, form, dtype, C, d):
    import sparse_rcnn_amd as scn
    from sparse_rcnn_amd.unet import residual_block
    coords, rules = cloud
    n = len(coords)
    flags = dict(bottleneck_divisor=d if "bottleneck_divisor" in FORMS[form] else 0,
                 main_path_relu=bool(FORMS[form].get("main_path_relu")))
    torch.manual_seed(17)
    block = residual_block(C, **flags).to(gpu)
    convs = [m for m in block.modules() if isinstance(m, scn.SubmanifoldConvolution)]
    assert len(convs) == R.n_convs(flags["bottleneck_divisor"])
    with torch.no_grad():
        for m in convs:
            m.bias.normal_(0, 0.1)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(n, C, generator=g)
    x = scn.InputLayer(3, torch.tensor([12, 12, 12]), mode=4)((torch.from_numpy(coords), feats.to(gpu), 2))
    assert torch.equal(x.features.cpu(), feats)                            # unique sites: rows in input order
    leaf = x.features.detach().requires_grad_()
    stored = leaf.to(torch.bfloat16) if dtype == "bf16" else leaf
    with _masks() as masks:
        y = block(scn.SparseConvNetTensor(stored, x.metadata, x.spatial_size)).features
    assert y.dtype == stored.dtype and len(masks) == len(convs)
    gy = torch.randn(n, C, generator=g)
    y.backward(gy.to(gpu).to(y.dtype))
    torch.cuda.synchronize()
    P = {}
    for v, m in enumerate(convs):
        P[f"u.conv{v}.weight"], P[f"u.conv{v}.bias"] = m.weight, m.bias
    Po, X = _f64(P), feats.double().requires_grad_()
    rounding = dict(q=_q, wq=_q) if dtype == "bf16" else {}
    x0 = _q(X) if dtype == "bf16" else X
    gyo = gy.to(torch.bfloat16).double() if dtype == "bf16" else gy.double()
    fr = O.FrozenReLU(masks)
    exp = R.unit(x0, Po, "u", rules, n, relu=fr, **flags, **rounding)
    assert fr.k == len(masks)
    exp.backward(gyo)
    name = f"unit {form} {dtype} C={C}"
    if dtype == "f32":
        with torch.no_grad():
            plain = R.unit(X, Po, "u", rules, n, **flags)
        _check(name + " forward", y, plain, FEAT_TOL, _scale_err)
    else:
        _check(name + " forward (scale)", y.float(), exp, BF16_FWD_SCALE, _scale_err)
        _check(name + " forward (L2)", y.float(), exp, BF16_FWD_L2)
    bound = L2_F32 if dtype == "f32" else L2_BF16
    _check(name + " grad input", leaf.grad, X.grad, bound)
    for k, p in P.items():
        _check(name + " grad " + k, p.grad, Po[k].grad, bound)


# ------------------------------------------------------------------------------------------------------ two-level SparseUNet
@pytest.fixture(scope="module")
def scene2k():
    from sparse_rcnn_amd.synthetic import make_batch
    coords, feats, size, bs, _ = make_batch(1, (64, 64, 32), 2_000, dup=1.15, seed=7)
    return coords, feats, size, O.OracleScene(coords.numpy())


def _net(gpu, form, dtype, seed=3):
    from sparse_rcnn_amd.unet import Backbone
    torch.manual_seed(seed)
    ch = (32, 64) if dtype == "bf16" else (16, 32)
    net = Backbone(7, ch, bf16_blocks="all" if dtype == "bf16" else False, **FORMS[form]).to(gpu)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    return net, ch


def _run(net, coords, feats, size, gpu, use_exec):
    from sparse_rcnn_amd.unet import SparseUNet
    SparseUNet.EXEC = use_exec
    try:
        for p in net.parameters():
            p.grad = None
        fin = feats.to(gpu).requires_grad_()
        out = net(coords, fin, size, 1)
        g = torch.Generator().manual_seed(11)
        outs, grads = [out.features], [torch.randn(out.features.shape, generator=g).to(gpu)]
        t = net.unet.interims[1]                                # a gradient arriving at the coarse encoder output too
        outs.append(t.features)
        grads.append(torch.randn(t.features.shape, generator=g).to(gpu).to(t.features.dtype))
        n_stage = _n_stage_nodes(out.features)
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
        return (n_stage, out.features.detach().clone(), [t.features.detach().clone() for t in net.unet.interims], fin.grad.clone(),
                [p.grad.clone() for p in net.parameters()])
    finally:
        SparseUNet.EXEC = True


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("form", list(FORMS))
def test_executor_is_bit_identical_to_the_module_path(gpu, scene2k, form, dtype):
    """Executor against layer-by-layer: output, encoder outputs, input gradient and every parameter gradient, all bits; the
    forward under torch.no_grad() (the lean slab layout) against the training forward, all bits."""
    from sparse_rcnn_amd import executor as EX
    coords, feats, size, _ = scene2k
    net, ch = _net(gpu, form, dtype)
    assert net.unet._exec_plan(), "the executor must cover this network"
    a = _run(net, coords, feats, size, gpu, True)
    b = _run(net, coords, feats, size, gpu, False)
    assert a[0] == 2 + 1 and b[0] == 0                           # the executor really ran / really did not
    assert torch.equal(a[1], b[1]), "output features"
    for l, (x, y) in enumerate(zip(a[2], b[2])):
        assert x.dtype == y.dtype and torch.equal(x, y), f"encoder output {l}"
    assert torch.equal(a[3], b[3]), "input-feature gradient"
    for (nm, _), x, y in zip(net.named_parameters(), a[4], b[4]):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y), f"gradient of {nm}"
    with torch.no_grad():
        out = net(coords, feats.to(gpu), size, 1)
    assert EX.LAST_FORWARD["lean"] is True and torch.equal(out.features, a[1])
    for x, t in zip(a[2], net.unet.interims):
        assert torch.equal(x, t.features)


@pytest.mark.parametrize("form", ["bottleneck", "both"])
def test_reference_plan_inner_widths_run_and_are_bit_identical(gpu, scene2k, form):
    """The reference's plan 32-48-64-80-96-112 at bottleneck_divisor=4: inner widths 8, 12, 16, 20, 24, 28 -- with the 8, 16, 32, 64
    of the benchmark plan every width the row GEMM, tile convolution and weight-gradient launchers meet.  fp32 (12, 20 and 28 are
    no multiples of 8); executor against layer-by-layer, all bits, gradients finite and not all zero."""
    from sparse_rcnn_amd.unet import Backbone
    coords, feats, size, _ = scene2k
    torch.manual_seed(9)
    net = Backbone(7, (32, 48, 64, 80, 96, 112), **FORMS[form]).to(gpu)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    a = _run(net, coords, feats, size, gpu, True)
    b = _run(net, coords, feats, size, gpu, False)
    assert a[0] == 6 + 5 and b[0] == 0
    assert torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    for (nm, _), x, y in zip(net.named_parameters(), a[4], b[4]):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0 and torch.equal(x, y), nm


@pytest.mark.parametrize("form", list(FORMS))
def test_dropin_control_flow_gives_the_backbone_bits(gpu, scene2k, form):
    """The units are the reference's nesting of scn modules, so the tree also runs the way the reference's containers drive it
    (unet.DropinBackbone: an encoder level called as one scn.Sequential, a decoder level as input stage / JoinTable /
    NetworkInNetwork / output stage with the deconvolution still pending when the units get it): no stage recognises the new
    units there, every layer computes on its own, and output and gradients are the executor's bit for bit."""
    from sparse_rcnn_amd.unet import DropinBackbone
    coords, feats, size, _ = scene2k
    net, ch = _net(gpu, form, "f32")
    ref = _run(net, coords, feats, size, gpu, True)
    for p in net.parameters():
        p.grad = None
    fin = feats.to(gpu).requires_grad_()
    out = DropinBackbone(net)(coords, fin, size, 1)
    assert _n_stage_nodes(out.features) == 0
    g = torch.Generator().manual_seed(11)                       # (the two upstream gradients of `_run`)
    gy = torch.randn(out.features.shape, generator=g).to(gpu)
    t = net.unet.interims[1].features
    torch.autograd.backward([out.features, t], [gy, torch.randn(t.shape, generator=g).to(gpu)])
    torch.cuda.synchronize()
    assert torch.equal(out.features, ref[1]) and torch.equal(fin.grad, ref[3])
    for (nm, p), y in zip(net.named_parameters(), ref[4]):
        assert torch.equal(p.grad, y), nm


@pytest.mark.parametrize("form", ["mainpath", "both"])
def test_the_output_slab_a_closing_relu_masks_by_outlives_the_callers_reference(gpu, scene2k, form):
    """The backward of a main-path unit that ends a stage masks by the stage's OUTPUT slab.  The stage keeps that slab for
    backward itself: a caller that drops the network's output before backward (bf16 storage does -- it widens the last slab and
    lets the stored one go) must get the gradients of the layer-by-layer path, whatever takes the freed block meanwhile."""
    from sparse_rcnn_amd.unet import SparseUNet
    coords, feats, size, _ = scene2k
    net, ch = _net(gpu, form, "f32")
    got = {}
    for use in (True, False):
        SparseUNet.EXEC = use
        try:
            for p in net.parameters():
                p.grad = None
            fin = feats.to(gpu).requires_grad_()
            out = net(coords, fin, size, 1)
            z = out.features * 2.0                              # (its backward keeps neither operand)
            shape = tuple(z.shape)
            assert _n_stage_nodes(z) == (3 if use else 0)
            del out
            torch.cuda.synchronize()
            junk = [torch.full(shape, float("nan"), device=gpu) for _ in range(16)]
            z.backward(torch.randn(shape, generator=torch.Generator().manual_seed(4)).to(gpu))
            torch.cuda.synchronize()
            del junk
            got[use] = [fin.grad.clone()] + [p.grad.clone() for p in net.parameters()]
        finally:
            SparseUNet.EXEC = True
    for x, y in zip(got[True], got[False]):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)


@pytest.mark.parametrize("form", list(FORMS))
def test_without_levels_the_network_falls_back(gpu, scene2k, form, monkeypatch):
    """executor.build_levels reports None for a scene with an empty level; the forward must then take the layer-by-layer path
    (no stage node) and give the executor's bits.  And a scene without any active site -- every level empty -- runs."""
    from sparse_rcnn_amd import executor as EX
    coords, feats, size, _ = scene2k
    net, ch = _net(gpu, form, "f32")
    ref = net(coords, feats.to(gpu), size, 1).features
    assert _n_stage_nodes(ref) == 3
    monkeypatch.setattr(EX, "build_levels", lambda md, size, n: None)
    out = net(coords, feats.to(gpu), size, 1).features
    assert _n_stage_nodes(out) == 0 and torch.equal(out, ref)
    monkeypatch.undo()
    empty = net(coords[:0], feats[:0].to(gpu).requires_grad_(), size, 1).features
    assert empty.shape == (0, ch[0]) and _n_stage_nodes(empty) == 0


@pytest.mark.parametrize("form", list(FORMS))
def test_reference_checkpoint_loads_and_the_forward_equals_the_restatement(gpu, scene2k, form):
    from sparse_rcnn_amd.unet import Backbone, reference_key_map
    coords, feats, size, scene = scene2k
    ch, flags = (16, 32), FORMS[form]
    P = R.init_params(7, ch, seed=23, **flags)
    # the checkpoint as the reference writes it: its key names under a prefix, SparseConvNet's grouped layout [fv, 1, nIn, nOut]
    sd = {"feature_extractor." + rk: (P[k].unsqueeze(1) if P[k].dim() == 3 else P[k]).clone()
          for rk, k in reference_key_map(len(ch), 2, **flags).items()}
    net = Backbone(7, ch, **flags).to(gpu)
    assert net.load_reference_state_dict(sd) == ([], [])
    with torch.no_grad():
        out = net(coords, feats.to(gpu), size, 1).features
        exp = R.unet_forward(scene, feats.double(), {k: v.double() for k, v in P.items()}, list(ch), **flags)
    _check(f"checkpoint {form} forward", out, exp, FEAT_TOL, _scale_err)


# ------------------------------------------------------------------------------------------------------------------ SceneStep
STEP_CASES = [("bottleneck", "f32"), ("mainpath", "f32"), ("both", "f32"), ("bottleneck", "bf16")]


@pytest.mark.parametrize("form,dtype", STEP_CASES, ids=[f"{f}-{t}" for f, t in STEP_CASES])
def test_scene_step_every_gradient_against_the_restatement(gpu, form, dtype):
    """One SceneStep('cfg2') on the smallest scene of the small-step tests (10 k voxels in 128 x 128 x 64) with the unit form
    switched on: every parameter gradient and the input gradient against the restatement, then a second step runs."""
    from sparse_rcnn_amd.trainstep import SceneStep
    flags, ch = FORMS[form], (32, 64, 128)
    job = SceneStep("cfg2", gpu, dtype=dtype, prefetch=False, seed=5, grad_seed=9, target=10_000, grid=(128, 128, 64), channels=ch,
                    lr=1e-3, **flags)
    unet = job.model.backbone.unet
    assert (unet.bottleneck_divisor, unet.main_path_relu) == (flags.get("bottleneck_divisor", 0), bool(flags.get("main_path_relu")))
    with torch.no_grad():
        g = torch.Generator().manual_seed(1)
        for p in job.model.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    with _masks() as masks:
        job.forward_backward()
    torch.cuda.synchronize()
    assert _n_stage_nodes(job.out.features) == 3 + 2             # the step executor ran
    n_relu = R.n_convs(flags.get("bottleneck_divisor", 0))      # one ReLU per convolution, whatever the form
    assert len(masks) == 5 * 2 * n_relu + 2
    named = unet.named_oracle_params()
    Po = _f64(named)
    feats = job.feats_cpu.double().requires_grad_()
    scene = O.OracleScene(job.coords_cpu.numpy())
    gy = job.upstream_grads()[0].cpu().double()
    rounding = dict(storage=_q, tile_weights=_q) if dtype == "bf16" else {}
    fr = O.FrozenReLU(masks)
    exp = R.unet_forward(scene, feats, Po, list(ch), relu=fr, **flags, **rounding)
    assert fr.k == len(masks)
    exp.backward(gy)
    name = f"step {form} {dtype}"
    if dtype == "f32":
        with torch.no_grad():
            plain = R.unet_forward(scene, feats, Po, list(ch), **flags)
        _check(name + " forward", job.out.features, plain, FEAT_TOL, _scale_err)
    else:
        _check(name + " forward (scale)", job.out.features, exp, BF16_FWD_SCALE, _scale_err)
        _check(name + " forward (L2)", job.out.features, exp, BF16_FWD_L2)
    bound = L2_F32 if dtype == "f32" else L2_BF16
    _check(name + " grad input", job.fin.grad, feats.grad, bound)
    for k, p in named.items():
        _check(name + " grad " + k, p.grad, Po[k].grad, bound)
    before = [p.detach().clone() for p in named.values()]
    job.step()
    job.step()
    job.finish()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(job.out.features).all())
    assert all(bool(torch.isfinite(p).all()) for p in named.values())
    assert any(not torch.equal(p.detach(), b) for p, b in zip(named.values(), before))
