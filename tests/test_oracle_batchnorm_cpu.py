"""CPU: the oracle's batch-norm U-Net (`O.unet_forward(batchnorm=True)`, the reference statement the cfg2-bn chain test in
tests/test_gpu_atsize.py checks the HIP step against) pinned to the composition of the oracle's single layers, its BN-ReLU
to the reference's dense-twin fixtures, and its parameter naming to the package's SparseUNet(batchnorm=True)."""
import os

import numpy as np
import pytest
import torch

from oracle import scn_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _scene(seed=3, grid=(10, 9, 8), n=260, dup=30):
    rng = np.random.default_rng(seed)
    cs = []
    for b in range(2):
        lin = rng.choice(grid[0] * grid[1] * grid[2], size=n, replace=False)
        p = np.stack(np.unravel_index(lin, grid), 1)
        p = np.concatenate([p, p[rng.integers(0, n, size=dup)]])
        cs.append(np.concatenate([p, np.full((len(p), 1), b)], 1))
    coords = np.concatenate(cs).astype(np.int64)
    feats = torch.from_numpy(rng.standard_normal((len(coords), 7))).double()
    return coords, feats


def _composed(scene, feats, P, ch, running, masks=None):
    """The cfg2-bn network written out with the oracle's single layers: BN-ReLU (O.batchnorm_relu_fwd, leak 0) in front of
    each bias-free SubM 3^3 convolution of a residual unit, everything else as in the plain U-Net."""
    masks = list(masks) if masks is not None else None

    def bn_relu(x, name):
        rm = running.setdefault(f"{name}.running_mean", torch.zeros(x.shape[1], dtype=x.dtype))
        rv = running.setdefault(f"{name}.running_var", torch.ones(x.shape[1], dtype=x.dtype))
        if masks is None:
            return O.batchnorm_relu_fwd(x, P[f"{name}.weight"], P[f"{name}.bias"], rm, rv, 1e-4, 0.9, 0.0, True)
        return O.batchnorm_affine(x, P[f"{name}.weight"], P[f"{name}.bias"], rm, rv, 1e-4, 0.9, True) * masks.pop(0)

    def relu(x):
        return torch.relu(x) if masks is None else x * masks.pop(0)

    def residual(x, prefix, level):
        rules, n = scene.subm_rules(level, 3), scene.n(level)
        for u in range(2):
            y = O.conv(bn_relu(x, f"{prefix}.res{u}.bn0"), P[f"{prefix}.res{u}.conv0.weight"], None, rules, n)
            y = O.conv(bn_relu(y, f"{prefix}.res{u}.bn1"), P[f"{prefix}.res{u}.conv1.weight"], None, rules, n)
            x = x + y
        return x

    x = O.input_layer_fwd(feats, scene.prow, scene.n(0), 4)
    skips = []
    for l in range(len(ch)):
        if l == 0:
            ident = [(np.arange(scene.n(0), dtype=np.int32),) * 2]
            x = O.conv(x, P["enc0.in.weight"], P["enc0.in.bias"], ident, scene.n(0))
        else:
            x = O.conv(x, P[f"enc{l}.in.weight"], P[f"enc{l}.in.bias"], scene.strided_rules(l - 1), scene.n(l))
        x = residual(x, f"enc{l}", l)
        skips.append(x)
    for l in range(len(ch) - 2, -1, -1):
        up = O.conv(relu(x), P[f"dec{l}.up.weight"], P[f"dec{l}.up.bias"], O.swap_rules(scene.strided_rules(l)), scene.n(l))
        x = torch.cat([up, skips[l]], 1) @ P[f"dec{l}.nin.weight"] + P[f"dec{l}.nin.bias"]
        x = residual(x, f"dec{l}", l)
    return x


def test_unet_forward_batchnorm_is_the_composition_of_the_oracle_layers():
    ch = [8, 12, 16]
    coords, feats = _scene()
    P = {k: v.double() for k, v in O.init_unet_params(7, ch, seed=2, batchnorm=True).items()}
    ran, ran2 = {}, {}
    y = O.unet_forward(O.OracleScene(coords), feats, P, ch, batchnorm=True, bn_running=ran)
    y2 = _composed(O.OracleScene(coords), feats, P, ch, ran2)
    assert y.shape == y2.shape and torch.allclose(y, y2, rtol=1e-12, atol=1e-12)
    assert set(ran) == set(ran2) and len(ran) == 2 * 4 * (2 * len(ch) - 1)       # 4 BN-ReLUs per level and direction
    for k in ran:
        assert torch.allclose(ran[k], ran2[k], rtol=1e-12, atol=1e-12), k
        # one step from (0, 1): running_mean = 0.1 * batch mean, running_var = 0.9 + 0.1 * unbiased batch variance
        assert (ran[k] != (0.0 if k.endswith("mean") else 1.0)).any(), k


def test_unet_forward_batchnorm_frozen_decisions_and_gradients():
    """Frozen decisions equal to the oracle's own give the same function; gamma, beta and the bias-free convolutions get
    gradients, and they equal those of the layer composition with the same masks."""
    ch = [8, 12]
    coords, feats = _scene(seed=5)
    P0 = {k: v.double() for k, v in O.init_unet_params(7, ch, seed=4, batchnorm=True).items()}
    scene = O.OracleScene(coords)
    masks = []

    def rec(x):
        masks.append(x > 0)
        return torch.relu(x)

    with torch.no_grad():
        plain = O.unet_forward(scene, feats, P0, ch, batchnorm=True, relu=rec)
    assert len(masks) == 4 * 3 + 1
    P = {k: v.clone().requires_grad_() for k, v in P0.items()}
    fr = O.FrozenReLU(masks)
    y = O.unet_forward(scene, feats, P, ch, batchnorm=True, relu=fr)
    assert fr.k == len(masks) and torch.allclose(y, plain, rtol=1e-12, atol=1e-12)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    y.backward(gy)
    Q = {k: v.clone().requires_grad_() for k, v in P0.items()}
    _composed(scene, feats, Q, ch, {}, masks=[m.double() for m in masks]).backward(gy)
    for k in P:
        assert P[k].grad is not None and P[k].grad.abs().max() > 0, k
        assert torch.allclose(P[k].grad, Q[k].grad, rtol=1e-10, atol=1e-12), k


def test_unet_forward_batchnorm_evaluation_reads_the_running_statistics():
    ch = [8, 12]
    coords, feats = _scene(seed=6)
    P = {k: v.double() for k, v in O.init_unet_params(7, ch, seed=1, batchnorm=True).items()}
    ran = {}
    O.unet_forward(O.OracleScene(coords), feats, P, ch, batchnorm=True, bn_running=ran)
    frozen = {k: v.clone() for k, v in ran.items()}
    y1 = O.unet_forward(O.OracleScene(coords), feats, P, ch, batchnorm=True, bn_running=ran, bn_training=False)
    assert all(torch.equal(ran[k], frozen[k]) for k in ran)
    y2 = O.unet_forward(O.OracleScene(coords), feats, P, ch, batchnorm=True, bn_running={}, bn_training=False)
    assert not torch.allclose(y1, y2)          # (0, 1) statistics are not the learnt ones


def test_unet_param_shapes_batchnorm():
    ch = [32, 64, 128, 256]
    plain = dict(O.unet_param_shapes(7, ch))
    bn = dict(O.unet_param_shapes(7, ch, batchnorm=True))
    res_bias = [k for k in plain if ".res" in k and k.endswith(".bias")]
    bn_names = [k for k in bn if ".bn" in k]
    assert len(res_bias) == 28 and not any(k in bn for k in res_bias)
    assert len(bn_names) == 2 * 28 and all(len(bn[k]) == 1 for k in bn_names)
    assert {k: v for k, v in bn.items() if ".bn" not in k} == {k: v for k, v in plain.items() if k not in res_bias}
    P = O.init_unet_params(7, ch, seed=0, batchnorm=True)
    gam = torch.cat([P[k] for k in bn_names if k.endswith("weight")])
    assert 0.5 < float(gam.min()) and float(gam.max()) < 1.5 and float(gam.std()) > 0.05


def test_sparse_unet_batchnorm_names_match_the_oracle():
    from sparse_rcnn_amd.unet import SparseUNet
    ch = (16, 32, 48)
    net = SparseUNet(7, ch, batchnorm=True)
    shapes = dict(O.unet_param_shapes(7, list(ch), batchnorm=True))
    own = net.named_oracle_params()
    assert set(own) == set(shapes)
    for k, p in own.items():
        assert p.numel() == int(np.prod(shapes[k])), k
    running = net.named_oracle_running_stats()
    assert set(running) == {k[:-len("weight")] + s for k in shapes if ".bn" in k and k.endswith("weight")
                            for s in ("running_mean", "running_var")}
    P = O.init_unet_params(7, list(ch), seed=3, batchnorm=True)
    net.load_oracle_params(P)
    assert all(torch.equal(own[k].detach().reshape(-1), P[k].reshape(-1)) for k in own)
    assert SparseUNet(7, ch).named_oracle_running_stats() == {}


def test_sparse_unet_refuses_batch_norm_on_a_padded_level():
    """identity_first with a level-0 width that is no multiple of 8 runs that level on zero-padded slabs; batch norm over
    them would normalise the pad column with a statistic that does not exist."""
    from sparse_rcnn_amd.unet import SparseUNet
    with pytest.raises(ValueError, match="batch norm"):
        SparseUNet(23, (23, 32, 48), batchnorm=True, identity_first=True)
    SparseUNet(24, (24, 32, 48), batchnorm=True, identity_first=True)          # no padding: allowed


@pytest.mark.parametrize("name", ["batchnorm_leaky0", "batchnorm_leaky0p2"])
def test_unet_bn_layer_equals_the_dense_twin(name):
    """The BN-ReLU as unet_forward(batchnorm=True) applies it -- relu(batchnorm_affine(x)) -- and the leaky form
    batchnorm_relu_fwd takes, against the reference's dense BatchNorm twins."""
    z = np.load(os.path.join(GOLD, f"dense_twin_{name}.npz"))
    X = torch.from_numpy(z["X"]).double().requires_grad_()
    ga = torch.from_numpy(z["param_0.weight"]).double().requires_grad_()
    be = torch.from_numpy(z["param_0.bias"]).double().requires_grad_()
    leak = float(z["leakiness"])
    rm, rv = torch.zeros(X.shape[1], dtype=torch.float64), torch.ones(X.shape[1], dtype=torch.float64)
    y = O.batchnorm_affine(X, ga, be, rm, rv, eps=float(z["eps"]), momentum=0.9)
    Y = torch.relu(y) if leak == 0 else torch.where(y > 0, y, y * leak)
    ref = torch.from_numpy(z["Y"]).double()
    assert float((Y.detach() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    for a, r in zip(torch.autograd.grad(Y, (X, ga, be), torch.from_numpy(z["dY"]).double()),
                    ("dX", "grad_0.weight", "grad_0.bias")):
        rr = torch.from_numpy(z[r]).double()
        assert float((a - rr).abs().max()) <= 1e-4 * float(rr.abs().max()), r
    n = X.shape[0]
    Xd = X.detach()
    assert torch.allclose(rm, 0.1 * Xd.mean(0), rtol=1e-12, atol=1e-15)
    assert torch.allclose(rv, 0.9 + 0.1 * Xd.var(0, unbiased=True), rtol=1e-12) and n > 1
