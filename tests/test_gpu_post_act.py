"""-m gpu: the reference's post-activation units, input-stage ReLUs and plain convolution blocks (unet.* with relu_first=,
drop_input_relu=, use_residuals=) on the device.

  * the fused end of a post-activation unit (SCN_OP_ADD_RELU, run as a one-op plan through scn_exec_run) against scn_relu_fwd(_bf16)
    followed by scn_add(_bf16), bit for bit, inside guarded buffers;
  * single units, encoder levels and a decoder level against the fixtures the reference's dense-mode factory produced
    (tests/golden/post_act_*.npz; the float64 restatement meets them exactly, tests/test_post_act_cpu.py);
  * every form as a three-level SparseUNet on a sparse two-sample scene: the step executor against the layer-by-layer path
    (all bits, fp32 and bf16 storage), forward-only against the training forward, and both against the float64 restatement
    with the device's own ReLU decisions;
  * a tree in the nesting the reference's factories build (plain scn modules, relu_first=False) takes the executor's stages and
    gives the layer-by-layer bits;
  * SceneStep with the switches: two steps, forward_only bit-equal to the training forward.

Bounds (the bars of tests/test_gpu_unit_forms.py): forward features within 1e-4 of the output's scale;
gradients with the ReLU masks the HIP forward recorded prescribed to the restatement (FrozenReLU) within 2e-5 relative L2 in
fp32 and 2e-2 in bf16 storage, there against the restatement with the same storage roundings."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # tests/post_act_restate.py
import post_act_restate as R                                             # noqa: E402
from oracle import scn_oracle as O                                       # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FEAT_TOL, L2_F32, L2_BF16 = 1e-4, 2e-5, 2e-2
BF16_FWD_SCALE, BF16_FWD_L2 = 2.0 ** -6, 1e-2
FORMS = {"pre_keep": dict(drop_input_relu=False), "post_keep": dict(relu_first=False, drop_input_relu=False),
         "post_drop": dict(relu_first=False), "plain_pre": dict(use_residuals=False),
         "plain_post": dict(use_residuals=False, relu_first=False),
         "post_bottleneck": dict(relu_first=False, bottleneck_divisor=4),
         "post_mainpath_keep": dict(relu_first=False, drop_input_relu=False, main_path_relu=True)}
GUARD, SENT = 512, 0xA5


class _Round(torch.autograd.Function):
    """bf16 storage of a slab at the restatement's own dtype, straight-through backward."""

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
    print(f"[post-act] {what}: {e:.3e} (bound {bound:.1e})")
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


# ------------------------------------------------------------------------------------------- SCN_OP_ADD_RELU, fp32 and bf16
class Buf:
    """`count` elements of `dtype` inside a sentinel-filled byte buffer; the data starts `off` elements past a 256-byte
    boundary.  `.t` views the data, `.ptr` is its address, `.intact()` says whether every byte outside it is untouched."""

    def __init__(self, dev, dtype, count, off=0, fill=None):
        isz = torch.empty((), dtype=dtype).element_size()
        self.lo = GUARD + off * isz
        self.hi = self.lo + int(count) * isz
        self.raw = torch.full((self.hi + GUARD,), SENT, dtype=torch.uint8, device=dev)
        assert self.raw.data_ptr() % 256 == 0
        self.t = self.raw[self.lo:self.hi].view(dtype)
        if fill is not None:
            self.t.copy_(fill.reshape(-1))
        self.ptr = self.raw.data_ptr() + self.lo

    def intact(self):
        return bool((self.raw[:self.lo] == SENT).all()) and bool((self.raw[self.hi:] == SENT).all())


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _planted(n, seed, shift):
    """randn (half of it negative) with +0, -0, NaN, a negative and a denormal at the positions i with (i + shift) % 11 < 5."""
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    special = torch.tensor([0.0, -0.0, float("nan"), -3.0, 1e-40])
    k = (torch.arange(n) + shift) % 11
    m = k < len(special)
    x[m] = special[k[m]]
    return x


ADD_RELU_CASES = [("f32", c) for c in (1, 7, 32)] + [("bf16", c) for c in (8, 40)]


@pytest.mark.parametrize("dtype,c", ADD_RELU_CASES, ids=[f"{t}-c{c}" for t, c in ADD_RELU_CASES])
def test_add_relu_has_the_bits_of_relu_then_add(gpu, dtype, c):
    """y = x + max(x1, 0) in one launch against the two launches it replaces, on the same operands: rows 0, 1, 37 and 4099 (the
    last one more than a block of 16-byte lanes, with a scalar tail at the odd widths), every pointer aligned and each in turn
    one element off (the scalar body), +0 / -0 / NaN / negatives / a denormal planted in both operands at positions that meet
    every pairing over the 11 x 11 grid of shifts 0 and 3.  x1 is bit-unchanged afterwards, nothing outside y is written; in
    place (y = x) gives the same bits."""
    from sparse_rcnn_amd import _lib as L, executor as EX
    lib = L.lib()
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    relu, add = (lib.scn_relu_fwd, lib.scn_add) if dtype == "f32" else (lib.scn_relu_fwd_bf16, lib.scn_add_bf16)
    scratch = Buf(gpu, torch.uint8, 256)

    def fused(x_ptr, t_ptr, y_ptr):
        EX.run_add_relu(x_ptr, t_ptr, y_ptr, n, c, dtype == "bf16", scratch.t)
    for n in (0, 1, 37, 4099):
        count = n * c
        X, T = _planted(count, 1, 0).to(td).to(gpu), _planted(count, 2, 3).to(td).to(gpu)
        for ox, ot, oy in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            x, t = Buf(gpu, td, count, ox, X), Buf(gpu, td, count, ot, T)
            y, r, want = Buf(gpu, td, count, oy), Buf(gpu, td, count), Buf(gpu, td, count, oy)
            fused(x.ptr, t.ptr, y.ptr)
            L.check(relu(t.ptr, count, r.ptr, L.stream()))
            L.check(add(x.ptr, r.ptr, count, want.ptr, L.stream()))
            torch.cuda.synchronize()
            assert torch.equal(_bits(y.t), _bits(want.t)), (n, ox, ot, oy)
            assert torch.equal(_bits(t.t), _bits(T.reshape(-1))) and torch.equal(_bits(x.t), _bits(X.reshape(-1))), "operands changed"
            assert x.intact() and t.intact() and y.intact() and scratch.intact(), ("guard", n, ox, ot, oy)
            if count >= 64:
                assert bool(torch.isnan(y.t.float()).any()) and bool((y.t.float() == X.float()).any())     # NaN from x; max(x1, 0) = 0
            fused(x.ptr, t.ptr, x.ptr)                                                                   # in place
            torch.cuda.synchronize()
            assert torch.equal(_bits(x.t), _bits(want.t)) and x.intact() and torch.equal(_bits(t.t), _bits(T.reshape(-1)))


# ------------------------------------------------------------------------------------- fixtures of the reference's dense factory
def _full_grid_input(gpu, vol, extra=None):
    """The fully active volume [B, C, X, Y, Z] as a sparse tensor on the device: (tensor, leaf features, coords)."""
    import sparse_rcnn_amd as scn
    coords = R.full_grid(vol.shape)
    rows = R.rows_of(torch.from_numpy(np.ascontiguousarray(vol))).float()
    x = scn.InputLayer(3, torch.tensor(vol.shape[2:]), mode=4)((torch.from_numpy(coords), rows.to(gpu), vol.shape[0]))
    assert np.array_equal(x.get_spatial_locations().numpy(), coords)      # unique sites: rows in input order
    leaf = x.features.detach().requires_grad_()
    return scn.SparseConvNetTensor(leaf, x.metadata, x.spatial_size), leaf, coords


def _rows_at(vol, coords):
    """Rows of a dense [B, C, X, Y, Z] array at the sites `coords` (x, y, z, batch)."""
    v = torch.from_numpy(np.ascontiguousarray(vol))
    c = torch.as_tensor(np.asarray(coords), dtype=torch.long)
    return v[c[:, 3], :, c[:, 0], c[:, 1], c[:, 2]]


def _load_units(unit_seq, P, prefix="u"):
    """Parameters named `<prefix>.res<u>.conv<v>` into a `unet.units(...)` Sequential (SparseUNet._res gives the names)."""
    from sparse_rcnn_amd.unet import SparseUNet
    own = {}
    SparseUNet._res(own, prefix, unit_seq)
    assert sorted(own) == sorted(k for k in P if ".res" in k)
    with torch.no_grad():
        for k, p in own.items():
            p.copy_(P[k].to(p.device))
    return own


def _grad_checks(name, own, G, leaf_grad, dX):
    _check(name + " grad input", leaf_grad, dX, L2_F32)
    for k, p in own.items():
        _check(name + " grad " + k, p.grad, G[k], L2_F32)


@pytest.mark.parametrize("name", ["plain", "bottleneck"])
def test_single_unit_against_the_references_fixture(gpu, name):
    from sparse_rcnn_amd import modules as M
    from sparse_rcnn_amd.unet import residual_block
    g = R.load(os.path.join(GOLD, f"post_act_unit_{name}.npz"))
    X, P, rules, n, flags, Y, dY, dX, G = R.fixture_unit(g)
    x, leaf, coords = _full_grid_input(gpu, g["X"])
    block = residual_block(X.shape[1], bottleneck_divisor=flags["bottleneck_divisor"], relu_first=False).to(gpu)
    own = _load_units(M.Sequential(block), {k.replace("u.", "u.res0."): v for k, v in P.items()})
    y = block(x).features
    _check(f"unit {name} forward", y, Y, FEAT_TOL, _scale_err)
    y.backward(dY.float().to(gpu))
    torch.cuda.synchronize()
    _grad_checks(f"unit {name}", own, {k.replace("u.", "u.res0."): v for k, v in G.items()}, leaf.grad, dX)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("name", ["pre_keep", "post_keep", "post_drop", "plain_pre", "plain_post"])
def test_encoder_level_against_the_references_fixture(gpu, name, stride):
    """Input stage + units as the builder nests them, called as ONE scn.Sequential (it runs as an executor stage)."""
    from sparse_rcnn_amd import modules as M
    from sparse_rcnn_amd.unet import input_stage, stage_layer, units
    g = R.load(os.path.join(GOLD, f"post_act_level_{name}_s{stride}.npz"))
    flags = R._flags(g)
    _, P, G, _, _, dX = R.fixture_level(g)
    x, leaf, coords = _full_grid_input(gpu, g["X"])
    head = M.SubmanifoldConvolution(3, 8, 16, 1, True) if stride == 1 else M.Convolution(3, 8, 16, (2, 2, 2), (2, 2, 2), True)
    level = M.Sequential(input_stage(head, False, flags["relu_first"], bool(g["drop_input_relu"])),
                         units(16, int(g["num_units"]), relu_first=flags["relu_first"], use_residuals=flags["use_residuals"])).to(gpu)
    own = _load_units(level[1], P)
    own["u.in.weight"], own["u.in.bias"] = stage_layer(level[0]).weight, stage_layer(level[0]).bias
    with torch.no_grad():
        own["u.in.weight"].copy_(P["u.in.weight"].to(gpu))
        own["u.in.bias"].copy_(P["u.in.bias"].to(gpu))
    out = level(x)
    assert _n_stage_nodes(out.features) == 1
    oc = out.get_spatial_locations().numpy()
    _check(f"level {name} s{stride} forward", out.features, _rows_at(g["Y"], oc), FEAT_TOL, _scale_err)
    out.features.backward(_rows_at(g["dY"], oc).float().to(gpu))
    torch.cuda.synchronize()
    _grad_checks(f"level {name} s{stride}", own, G, leaf.grad, dX)


def test_decoder_level_against_the_references_fixture(gpu):
    """Deconvolution -> ReLU, JoinTable, NetworkInNetwork, one post-activation unit, driven as the reference's
    SkipConnectionReuniter drives them (four calls; the level runs as one executor stage)."""
    import sparse_rcnn_amd as scn
    from sparse_rcnn_amd import modules as M
    from sparse_rcnn_amd.unet import input_stage, stage_layer, units
    g = R.load(os.path.join(GOLD, "post_act_reunite.npz"))
    _, _, P, G, _, _, _, dS = R.fixture_reunite(g)
    skip, sleaf, coords = _full_grid_input(gpu, g["S"])
    probe = M.Convolution(3, 8, 16, (2, 2, 2), (2, 2, 2), False).to(gpu)(skip)           # the coarse grid and its rules
    cc = probe.get_spatial_locations().numpy()
    cleaf = _rows_at(g["X"], cc).float().to(gpu).requires_grad_()
    xc = scn.SparseConvNetTensor(cleaf, probe.metadata, probe.spatial_size)
    up = input_stage(M.Deconvolution(3, 16, 8, (2, 2, 2), (2, 2, 2), True), False, False).to(gpu)
    nin, un = M.NetworkInNetwork(16, 8, True).to(gpu), units(8, 1, relu_first=False).to(gpu)
    own = _load_units(un, P)
    own.update({"u.up.weight": stage_layer(up).weight, "u.up.bias": stage_layer(up).bias, "u.nin.weight": nin.weight,
                "u.nin.bias": nin.bias})
    with torch.no_grad():
        for k in ("u.up.weight", "u.up.bias", "u.nin.weight", "u.nin.bias"):
            own[k].copy_(P[k].to(gpu).view_as(own[k]))
    out = un(nin(M.JoinTable()([up(xc), skip])))
    assert _n_stage_nodes(out.features) == 1
    assert np.array_equal(out.get_spatial_locations().numpy(), coords)
    _check("reunite forward", out.features, R.rows_of(torch.from_numpy(g["Y"])), FEAT_TOL, _scale_err)
    out.features.backward(R.rows_of(torch.from_numpy(g["dY"])).float().to(gpu))
    torch.cuda.synchronize()
    _check("reunite grad coarse input", cleaf.grad, _rows_at(g["dX"], cc), L2_F32)
    _check("reunite grad skip", sleaf.grad, dS, L2_F32)
    for k, p in own.items():
        _check("reunite grad " + k, p.grad, G[k].view_as(p), L2_F32)


# ------------------------------------------------------------------------------------------ every form through SparseUNet
@pytest.fixture(scope="module")
def scene3k():
    """Two samples in 64 x 64 x 32, ~3 000 active voxels together, the second a tenth of the first; the row count of no level
    is a multiple of 16 (so none of 256)."""
    from sparse_rcnn_amd.synthetic import make_scene
    cs, fs = [], []
    for b, target in enumerate((2_700, 300)):
        p, f, _ = make_scene((64, 64, 32), target, 1.15, 31 + b, False)
        cs.append(np.concatenate([p, np.full((len(p), 1), b, np.int64)], 1))
        fs.append(f[:, :7])
    coords = torch.from_numpy(np.concatenate(cs))
    feats = torch.from_numpy(np.ascontiguousarray(np.concatenate(fs)))
    scene = O.OracleScene(coords.numpy())
    scene.strided_rules(0), scene.strided_rules(1)
    ns = [scene.n(l) for l in range(3)]
    assert 2_500 < ns[0] < 3_500 and all(n % 16 for n in ns), ns
    return coords, feats, torch.tensor((64, 64, 32)), scene


def _channels(form, dtype):
    return (32, 64, 128) if (form == "post_bottleneck" and dtype == "bf16") else (8, 16, 32)      # bf16: inner widths 8, 16, 32


def _net(gpu, form, dtype, seed=3):
    from sparse_rcnn_amd.unet import Backbone
    torch.manual_seed(seed)
    ch = _channels(form, dtype)
    net = Backbone(7, ch, bf16_blocks="all" if dtype == "bf16" else False, **FORMS[form]).to(gpu)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    return net, ch


def _run(net, coords, feats, size, gpu, use_exec, record=False):
    from sparse_rcnn_amd import functional as F
    from sparse_rcnn_amd.unet import SparseUNet
    SparseUNet.EXEC = use_exec
    try:
        for p in net.parameters():
            p.grad = None
        fin = feats.to(gpu).requires_grad_()
        if record:
            F.RELU_RECORD = []
        out = net(coords, fin, size, 2)
        masks, F.RELU_RECORD = F.RELU_RECORD, None
        g = torch.Generator().manual_seed(11)
        gy = torch.randn(out.features.shape, generator=g)
        outs, grads = [out.features], [gy.to(gpu)]
        t = net.unet.interims[1]                                # a gradient arriving at an encoder output too
        g1 = torch.randn(t.features.shape, generator=g)
        outs.append(t.features)
        grads.append(g1.to(gpu).to(t.features.dtype))
        n_stage = _n_stage_nodes(out.features)
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
        return dict(n_stage=n_stage, out=out.features.detach().clone(), interims=[t.features.detach().clone() for t in net.unet.interims],
                    din=fin.grad.clone(), grads=[p.grad.clone() for p in net.parameters()], masks=masks, gy=gy, g1=g1)
    finally:
        F.RELU_RECORD = None
        SparseUNet.EXEC = True


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("form", list(FORMS))
def test_executor_is_bit_identical_to_the_module_path(gpu, scene3k, form, dtype):
    """The executor adds no arithmetic of its own: output, encoder outputs, input gradient and every parameter gradient, all
    bits, and the same ReLU decisions in the same order; the forward under torch.no_grad() (the lean slab layout) against the
    training forward, all bits."""
    from sparse_rcnn_amd import executor as EX
    coords, feats, size, _ = scene3k
    net, ch = _net(gpu, form, dtype)
    assert net.unet._exec_plan(), "the executor must cover this network"
    a = _run(net, coords, feats, size, gpu, True, record=True)
    b = _run(net, coords, feats, size, gpu, False, record=True)
    assert a["n_stage"] == 3 + 2 and b["n_stage"] == 0            # the executor really ran / really did not
    assert a["out"].dtype == b["out"].dtype and torch.equal(a["out"], b["out"]), "output features"
    for l, (x, y) in enumerate(zip(a["interims"], b["interims"])):
        assert x.dtype == y.dtype and torch.equal(x, y), f"encoder output {l}"
    assert torch.equal(a["din"], b["din"]), "input-feature gradient"
    for (nm, _), x, y in zip(net.named_parameters(), a["grads"], b["grads"]):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0 and torch.equal(x, y), f"gradient of {nm}"
    assert len(a["masks"]) == len(b["masks"]) > 0
    for k, (x, y) in enumerate(zip(a["masks"], b["masks"])):
        assert x.shape == y.shape and torch.equal(x, y), f"ReLU mask {k}"
    with torch.no_grad():
        out = net(coords, feats.to(gpu), size, 2)
    assert EX.LAST_FORWARD["lean"] is True and torch.equal(out.features, a["out"])
    for x, t in zip(a["interims"], net.unet.interims):
        assert torch.equal(x, t.features)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("form", list(FORMS))
def test_network_against_the_restatement_with_the_devices_relu_masks(gpu, scene3k, form, dtype):
    coords, feats, size, scene = scene3k
    net, ch = _net(gpu, form, dtype)
    a = _run(net, coords, feats, size, gpu, True, record=True)
    named = net.unet.named_oracle_params()
    Po = _f64(named)
    X = feats.double().requires_grad_()
    rounding = dict(storage=_q, tile_weights=_q) if dtype == "bf16" else {}
    fr = O.FrozenReLU(a["masks"])
    inter = []
    exp = R.unet_forward(scene, X, Po, list(ch), relu=fr, interims=inter, **FORMS[form], **rounding)
    assert fr.k == len(a["masks"])
    g1 = a["g1"].to(torch.bfloat16).double() if dtype == "bf16" else a["g1"].double()
    gy = a["gy"].to(torch.bfloat16).double() if dtype == "bf16" else a["gy"].double()     # (the network's last cast rounds it)
    torch.autograd.backward([exp, inter[1]], [gy, g1])
    name = f"net {form} {dtype}"
    if dtype == "f32":
        with torch.no_grad():
            plain = R.unet_forward(scene, X, Po, list(ch), **FORMS[form])
        _check(name + " forward", a["out"], plain, FEAT_TOL, _scale_err)
    else:
        _check(name + " forward (scale)", a["out"], exp, BF16_FWD_SCALE, _scale_err)
        _check(name + " forward (L2)", a["out"], exp, BF16_FWD_L2)
    bound = L2_F32 if dtype == "f32" else L2_BF16
    _check(name + " grad input", a["din"], X.grad, bound)
    grads = dict(zip([n for n, _ in net.named_parameters()], a["grads"]))
    by_param = {id(p): n for n, p in net.named_parameters()}
    for k, p in named.items():
        _check(name + " grad " + k, grads[by_param[id(p)]], Po[k].grad, bound)


@pytest.mark.parametrize("form", ["post_keep", "plain_post"])
def test_reference_checkpoint_loads_and_the_forward_equals_the_restatement(gpu, scene3k, form):
    from sparse_rcnn_amd.unet import Backbone, reference_key_map
    coords, feats, size, scene = scene3k
    ch, flags = (8, 16, 32), FORMS[form]
    P = R.init_params(7, ch, seed=23, **flags)
    sd = {"feature_extractor." + rk: (P[k].unsqueeze(1) if P[k].dim() == 3 else P[k]).clone()
          for rk, k in reference_key_map(len(ch), 2, **flags).items()}
    net = Backbone(7, ch, **flags).to(gpu)
    assert net.load_reference_state_dict(sd) == ([], [])
    with torch.no_grad():
        out = net(coords, feats.to(gpu), size, 2).features
        exp = R.unet_forward(scene, feats.double(), {k: v.double() for k, v in P.items()}, list(ch), **flags)
    _check(f"checkpoint {form} forward", out, exp, FEAT_TOL, _scale_err)


# ------------------------------------------------------------------------------------ a tree in the reference's own nesting
class _Interims(torch.nn.Sequential):
    """Control flow of the reference's SequentialInterims (custom_container.py:5-12)."""

    def forward(self, x):
        outs = []
        for m in self:
            x = m(x)
            outs.append(x)
        return outs


class _Reuniter(torch.nn.Module):
    """Control flow of the reference's SkipConnectionReuniter (custom_container.py:70-83)."""

    def __init__(self, input_stage, combiner, channel_changer, output_stage):
        super().__init__()
        self.input_stage, self.combiner, self.channel_changer, self.output_stage = input_stage, combiner, channel_changer, output_stage

    def forward(self, x, skip):
        return self.output_stage(self.channel_changer(self.combiner([self.input_stage(x), skip])))


class _FactoryTree(torch.nn.Module):
    """The tree the reference's factories build for sparse + U-Net with relu_first=False (and drop_input_relu /
    use_residuals as given), from the package's PUBLIC scn surface only -- scn.ReLU() and scn.AddTable() as the factory calls
    them, every input stage an scn.Sequential -- under the reference's attribute names, so that its state_dict keys can be
    held against the key list the reference's own FeatureExtractor recorded (tests/golden/post_act_keys.json)."""

    def __init__(self, cin, channels, drop_input_relu, use_residuals):
        super().__init__()
        import sparse_rcnn_amd as scn

        def conv3(c):
            return scn.SubmanifoldConvolution(3, c, c, 3, True)

        def unit_stage(c):
            if not use_residuals:
                return scn.Sequential(conv3(c), scn.ReLU(), conv3(c), scn.ReLU())
            return scn.Sequential(*[scn.Sequential(scn.ConcatTable(scn.Identity(), scn.Sequential(conv3(c), scn.ReLU(), conv3(c), scn.ReLU())),
                                                   scn.AddTable()) for _ in range(2)])

        def stage(layer, drop):
            return scn.Sequential(layer) if drop else scn.Sequential(layer, scn.ReLU())
        levels = []
        for l, c in enumerate(channels):
            head = (scn.SubmanifoldConvolution(3, cin, c, 1, True) if l == 0
                    else scn.Convolution(3, channels[l - 1], c, (2, 2, 2), (2, 2, 2), True))
            levels.append(scn.Sequential(stage(head, drop_input_relu), unit_stage(c)))
        self.main_network = _Interims(*levels)
        self.unet = torch.nn.Module()
        self.unet.module_list = torch.nn.ModuleList([
            _Reuniter(stage(scn.Deconvolution(3, channels[l + 1], channels[l], (2, 2, 2), (2, 2, 2), True), False), scn.JoinTable(),
                      scn.NetworkInNetwork(2 * channels[l], channels[l], True), unit_stage(channels[l]))
            for l in range(len(channels) - 2, -1, -1)])

    def forward(self, coords, feats, size, bs):
        import sparse_rcnn_amd as scn
        x = scn.InputLayer(3, size, mode=4)((coords, feats, bs))
        *skips, x = self.main_network(x)
        self.interims = skips + [x]
        for m, skip in zip(self.unet.module_list, skips[::-1]):
            x = m(x, skip)
        return x


@pytest.mark.parametrize("name", ["post_keep", "post_drop", "plain_post"])
def test_a_tree_in_the_references_nesting_takes_the_stages(gpu, scene3k, name):
    """Stages on against stages off (SCN_TREE_STAGES): the stage count, and output, encoder outputs, input gradient and every
    parameter gradient bit for bit."""
    from sparse_rcnn_amd import modules as M
    coords, feats, size, _ = scene3k
    flags = FORMS[name]
    with open(os.path.join(GOLD, "post_act_keys.json")) as f:
        fx = json.load(f)[name]
    wide = _FactoryTree(7, fx["channels"], flags.get("drop_input_relu", True), flags.get("use_residuals", True))
    assert {k: list(v.shape) for k, v in wide.state_dict().items()} == fx["keys"]        # the reference's tree, key for key
    del wide
    torch.manual_seed(4)
    ch = (8, 16, 32)
    tree = _FactoryTree(7, ch, flags.get("drop_input_relu", True), flags.get("use_residuals", True)).to(gpu)
    with torch.no_grad():
        for p in tree.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.05)
    res = []
    try:
        for stages in (True, False):
            M.TREE_STAGES = stages
            M.STAGE_STATS.update(enc=0, dec=0, layerwise_units=0)
            for p in tree.parameters():
                p.grad = None
            fin = feats.to(gpu).requires_grad_()
            out = tree(coords, fin, size, 2)
            g = torch.Generator().manual_seed(11)
            outs = [out.features] + [t.features for t in tree.interims[1:]]
            grads = [torch.randn(o.shape, generator=g).to(gpu) for o in outs]
            n_stage = _n_stage_nodes(out.features)
            torch.autograd.backward(outs, grads)
            torch.cuda.synchronize()
            if stages:
                assert M.STAGE_STATS == dict(enc=3, dec=2, layerwise_units=0) and n_stage == 5, (M.STAGE_STATS, n_stage)
            else:
                assert M.STAGE_STATS["enc"] == 0 and M.STAGE_STATS["dec"] == 0 and n_stage == 0
            res.append((out.features.detach().clone(), [t.features.detach().clone() for t in tree.interims], fin.grad.clone(),
                        [p.grad.clone() for p in tree.parameters()]))
    finally:
        M.TREE_STAGES = True
    a, b = res
    assert torch.equal(a[0], b[0]), "output features"
    for l, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(x, y), f"encoder output {l}"
    assert torch.equal(a[2], b[2]), "input-feature gradient"
    for (n, _), x, y in zip(tree.named_parameters(), a[3], b[3]):
        assert float(x.abs().max()) > 0 and torch.equal(x, y), f"gradient of {n}"


# ------------------------------------------------------------------------------------------------------------------ SceneStep
STEP_FLAGS = {"post_keep": dict(relu_first=False, drop_input_relu=False), "plain": dict(use_residuals=False)}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("form", list(STEP_FLAGS))
def test_scene_step_takes_two_steps_and_its_forward_only_is_the_training_forward(gpu, form, dtype):
    from sparse_rcnn_amd import executor as EX
    from sparse_rcnn_amd.trainstep import SceneStep
    flags = STEP_FLAGS[form]
    job = SceneStep("cfg2", gpu, dtype=dtype, prefetch=False, seed=5, grad_seed=9, target=10_000, grid=(128, 128, 64),
                    channels=(32, 64, 128), lr=1e-3, **flags)
    unet = job.model.backbone.unet
    assert (unet.relu_first, unet.drop_input_relu, unet.use_residuals) == (
        flags.get("relu_first", True), flags.get("drop_input_relu", True), flags.get("use_residuals", True))
    job.forward_backward()
    torch.cuda.synchronize()
    assert _n_stage_nodes(job.out.features) == 3 + 2             # the step executor ran
    ref = job.out.features.detach().clone()
    inter = [t.features.detach().clone() for t in unet.interims]
    assert bool(torch.isfinite(ref).all())
    for n, p in unet.named_oracle_params().items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
    out, _ = job.forward_only()
    assert EX.LAST_FORWARD["lean"] is True and torch.equal(out.features, ref)
    for x, t in zip(inter, unet.interims):
        assert torch.equal(x, t.features)
    before = [p.detach().clone() for p in unet.parameters()]
    job.step()
    job.step()
    job.finish()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(job.out.features).all())
    assert all(bool(torch.isfinite(p).all()) for p in unet.parameters())
    assert any(not torch.equal(p.detach(), b) for p, b in zip(unet.parameters(), before))
