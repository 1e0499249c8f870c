"""Restatement of the forms sparse_rcnn_amd.unet builds for relu_first=False, drop_input_relu=False and use_residuals=False
(module_factory.py:127-218 units, :438-486 input stages, :489-578 levels), in torch on the CPU at the dtype of its operands (the
tests use float64), on top of the oracle's primitives and tests/unit_forms_restate.py, which keeps the relu_first=True units.

    residual unit, relu_first=False     y = x + act(K2(act(K1(x))))                       (main_path_relu: as relu_first=True)
      with bottleneck_divisor = d       y = x + act(N2(act(K(act(N1(x))))))
    input stage                         act -> layer | layer -> act | layer               (relu_first | not | ReLU dropped)
    plain blocks, use_residuals=False   [act, K] * n | [K, act] * n                       (relu_first | not)
    encoder level                       input stage (ReLU dropped with drop_input_relu) + units
    decoder level                       input stage around the Deconvolution (never dropped) -> JoinTable -> NiN -> units

Pinned against fixtures the reference's own dense-mode factory produced (tests/golden/post_act_*.npz,
tests/test_post_act_cpu.py); the GPU tests (tests/test_gpu_post_act.py) compare the HIP path against it.

`relu` is called once per ReLU in the order the HIP forward applies (and records) them: an input stage's ReLU where it stands,
inside a unit from the input to the output, the activation that closes a post-activation branch last.
Parameter names are `SparseUNet.named_oracle_params`; a plain block is `<level>.res<u>.conv0`."""
import numpy as np
import torch

import unit_forms_restate as R
from oracle import scn_oracle as O

conv_weight_to_scn, full_grid, rows_of = R.conv_weight_to_scn, R.full_grid, R.rows_of


def deconv_weight_to_scn(w):
    """torch ConvTranspose3d weight [Cin, Cout, a, b, c] -> scn Deconvolution layout [(a*2+b)*2+c, Cin, Cout]."""
    ci, co = w.shape[:2]
    return w.permute(2, 3, 4, 0, 1).reshape(-1, ci, co).contiguous()


def n_convs(bottleneck_divisor=0, use_residuals=True):
    return 1 if not use_residuals else R.n_convs(bottleneck_divisor)


def unit(x, P, prefix, rules, n, bottleneck_divisor=0, main_path_relu=False, relu_first=True, use_residuals=True, relu=torch.relu,
         q=None, wq=None):
    """One unit on `n` rows.  q: rounding of every STORED slab (bf16 storage; None: none); wq: rounding of the weights of the
    3^3 convolutions (their bf16 tile image).  A post-activation unit stores its branch, applies the activation to the stored
    slab (exact) and rounds the sum with the skip once."""
    if use_residuals and (relu_first or main_path_relu):
        return R.unit(x, P, prefix, rules, n, bottleneck_divisor, main_path_relu, relu, q, wq)
    q = q or (lambda t: t)
    wq = wq or (lambda t: t)
    W = lambda v: P[f"{prefix}.conv{v}.weight"]
    b = lambda v: P[f"{prefix}.conv{v}.bias"]
    if not use_residuals:
        if relu_first:
            return q(O.conv(relu(x), wq(W(0)), b(0), rules, n))
        return relu(q(O.conv(x, wq(W(0)), b(0), rules, n)))
    ident = [(np.arange(n, dtype=np.int32),) * 2]
    if bottleneck_divisor:
        h = q(O.conv(x, W(0), b(0), ident, n))
        h = q(O.conv(relu(h), wq(W(1)), b(1), rules, n))
        h = q(O.conv(relu(h), W(2), b(2), ident, n))
    else:
        h = q(O.conv(x, wq(W(0)), b(0), rules, n))
        h = q(O.conv(relu(h), wq(W(1)), b(1), rules, n))
    return q(x + relu(h))


def input_stage(x, W, b, rules, n_out, relu_first=True, drop_relu=False, relu=torch.relu, q=None):
    """act -> layer | layer -> act | layer alone; the layer's result is stored (q), the trailing activation acts on it."""
    q = q or (lambda t: t)
    if drop_relu:
        return q(O.conv(x, W, b, rules, n_out))
    if relu_first:
        return q(O.conv(relu(x), W, b, rules, n_out))
    return relu(q(O.conv(x, W, b, rules, n_out)))


def units(x, P, prefix, rules, n, num_units=2, **kw):
    for u in range(num_units):
        x = unit(x, P, f"{prefix}.res{u}", rules, n, **kw)
    return x


def param_shapes(cin, channels, bottleneck_divisor=0, main_path_relu=False, use_residuals=True, num_units=2, **_):
    """Ordered (name, shape) list: R.param_shapes with one convolution per plain block."""
    if use_residuals:
        return R.param_shapes(cin, channels, bottleneck_divisor, main_path_relu, num_units)
    out = []
    for name, shape in R.param_shapes(cin, channels, 0, False, num_units):
        if ".conv1." not in name:
            out.append((name, shape))
    return out


def init_params(cin, channels, seed=0, dtype=torch.float32, bias_std=0.05, **flags):
    g = torch.Generator().manual_seed(seed)
    P = {}
    for name, shape in param_shapes(cin, channels, **flags):
        if name.endswith("weight"):
            fan = shape[-2] * (shape[0] if len(shape) == 3 else 1)
            P[name] = (torch.randn(shape, generator=g, dtype=torch.float64) * (2.0 / fan) ** 0.5).to(dtype)
        else:
            P[name] = (torch.randn(shape, generator=g, dtype=torch.float64) * bias_std).to(dtype)
    return P


def unet_forward(scene, feats_pts, P, channels, bottleneck_divisor=0, main_path_relu=False, relu_first=True, drop_input_relu=True,
                 use_residuals=True, relu=None, storage=None, tile_weights=None, interims=None, num_units=2):
    """R.unet_forward with every switch.  storage / tile_weights as there: stored slabs after the first layer (level 0's input
    stage runs in fp32 and its result is stored once, behind its activation), weights of the layers on the bf16 tile kernel."""
    relu = torch.relu if relu is None else relu
    q = storage if storage is not None else (lambda t: t)
    wq = tile_weights if tile_weights is not None else (lambda t: t)
    kw = dict(bottleneck_divisor=bottleneck_divisor, main_path_relu=main_path_relu, relu_first=relu_first,
              use_residuals=use_residuals, relu=relu, q=q, wq=wq, num_units=num_units)
    x = O._InputFn.apply(feats_pts, scene)
    skips, L = [], len(channels)
    for l in range(L):
        if l == 0:
            ident = [(np.arange(scene.n(0), dtype=np.int32),) * 2]
            x = q(input_stage(x, P["enc0.in.weight"], P["enc0.in.bias"], ident, scene.n(0), relu_first, drop_input_relu, relu))
        else:
            x = input_stage(x, wq(P[f"enc{l}.in.weight"]), P[f"enc{l}.in.bias"], scene.strided_rules(l - 1), scene.n(l), relu_first,
                            drop_input_relu, relu, q)
        x = units(x, P, f"enc{l}", scene.subm_rules(l, 3), scene.n(l), **kw)
        skips.append(x)
    if interims is not None:
        interims.extend(skips)
    for l in range(L - 2, -1, -1):
        rules = O.swap_rules(scene.strided_rules(l))
        up = input_stage(x, P[f"dec{l}.up.weight"], P[f"dec{l}.up.bias"], rules, scene.n(l), relu_first, False, relu, q)
        x = q(torch.cat([up, skips[l]], 1) @ P[f"dec{l}.nin.weight"] + P[f"dec{l}.nin.bias"])
        x = units(x, P, f"dec{l}", scene.subm_rules(l, 3), scene.n(l), **kw)
    return x


# ---- the dense-twin fixtures (tests/golden/make_post_act_golden.py) ------------------------------------------------------------
def load(path):
    """A post_act_*.npz as {name: float64 array}: the integers of make_post_act_golden.pack times their step (exact)."""
    z = np.load(path)
    return {k: (z[k].astype(np.float64) * float(z[k + "__step"]) if k + "__step" in z.files else z[k])
            for k in z.files if not k.endswith("__step")}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _flags(g):
    return dict(bottleneck_divisor=int(g["bottleneck_divisor"]), main_path_relu=bool(g["main_path_relu"]),
                relu_first=bool(g["relu_first"]), use_residuals=bool(g["use_residuals"]))


def _unit_params(g, prefix, names, flags):
    """Parameters and gradients of the units under the state_dict prefix `prefix`, in this package's names and layout."""
    P, G = {}, {}
    if flags["use_residuals"]:
        blocks = sorted({int(k[len("param_" + prefix):].split(".")[0]) for k in names if k.startswith("param_" + prefix)})
        for u, blk in enumerate(blocks):
            stem = f"{prefix}{blk}.inner_block."
            idx = sorted({int(k[len("param_" + stem):].split(".")[0]) for k in names if k.startswith("param_" + stem)})
            assert len(idx) == n_convs(flags["bottleneck_divisor"])
            for v, i in enumerate(idx):
                for dst, pre in ((P, "param_"), (G, "grad_")):
                    dst[f"u.res{u}.conv{v}.weight"] = conv_weight_to_scn(_t(g[f"{pre}{stem}{i}.weight"]))
                    dst[f"u.res{u}.conv{v}.bias"] = _t(g[f"{pre}{stem}{i}.bias"])
        return P, G, len(blocks)
    idx = sorted({int(k[len("param_" + prefix):].split(".")[0]) for k in names if k.startswith("param_" + prefix)})
    for u, i in enumerate(idx):
        for dst, pre in ((P, "param_"), (G, "grad_")):
            dst[f"u.res{u}.conv0.weight"] = conv_weight_to_scn(_t(g[f"{pre}{prefix}{i}.weight"]))
            dst[f"u.res{u}.conv0.bias"] = _t(g[f"{pre}{prefix}{i}.bias"])
    return P, G, len(idx)


def fixture_unit(g):
    """A post_act_unit_*.npz -> (X rows, P, rules, n, flags, Y rows, dY rows, dX rows, G), parameters as `u.conv<v>`."""
    flags = _flags(g)
    idx = sorted({int(k.split(".")[1]) for k in g if k.startswith("param_inner_block.")})
    assert len(idx) == n_convs(flags["bottleneck_divisor"])
    P, G = {}, {}
    for v, i in enumerate(idx):
        for dst, pre in ((P, "param_"), (G, "grad_")):
            dst[f"u.conv{v}.weight"] = conv_weight_to_scn(_t(g[f"{pre}inner_block.{i}.weight"]))
            dst[f"u.conv{v}.bias"] = _t(g[f"{pre}inner_block.{i}.bias"])
    coords = full_grid(g["X"].shape)
    return (rows_of(_t(g["X"])), P, O.subm_rulebook(coords, 3)[1], len(coords), flags, rows_of(_t(g["Y"])), rows_of(_t(g["dY"])),
            rows_of(_t(g["dX"])), G)


class FullGrid:
    """Index state of a fully active fine grid and its 2^3/2 coarse grid, with the row permutation between the oracle's coarse
    row numbering and the dense volume's (`coarse_rows(volume)` gives the volume's rows in the oracle's order)."""

    def __init__(self, fine_shape):
        self.fine = full_grid(fine_shape)
        self.n_fine = len(self.fine)
        self.fine_rules = O.subm_rulebook(self.fine, 3)[1]
        rb = O.strided_rulebook(self.fine, 2)
        self.down = rb["rules"]
        cc = np.asarray(rb["coords"], np.int64)
        self.n_coarse = len(cc)
        self.coarse_rules = O.subm_rulebook(cc, 3)[1]
        B, _, X, Y, Z = fine_shape
        self.perm = torch.from_numpy(((cc[:, 3] * (X // 2) + cc[:, 0]) * (Y // 2) + cc[:, 1]) * (Z // 2) + cc[:, 2])

    def coarse_rows(self, volume):
        return rows_of(volume)[self.perm]


def level_forward(g, X, P, relu=torch.relu):
    """The encoder level of a post_act_level_*.npz on rows X (fine rows at stride 2) -> output rows in the oracle's order."""
    flags, stride = _flags(g), int(g["stride"])
    drop = bool(g["drop_input_relu"])
    shape = g["X"].shape
    if stride == 1:
        coords = full_grid(shape)
        n = len(coords)
        ident = [(np.arange(n, dtype=np.int32),) * 2]
        x = input_stage(X, P["u.in.weight"], P["u.in.bias"], ident, n, flags["relu_first"], drop, relu)
        rules = O.subm_rulebook(coords, 3)[1]
    else:
        fg = FullGrid(shape)
        n, rules = fg.n_coarse, fg.coarse_rules
        x = input_stage(X, P["u.in.weight"], P["u.in.bias"], fg.down, n, flags["relu_first"], drop, relu)
    return units(x, P, "u", rules, n, num_units=int(g["num_units"]), relu=relu, **flags)


def fixture_level(g):
    """A post_act_level_*.npz -> (X rows, P, G, Y rows, dY rows, dX rows), coarse rows in the oracle's order."""
    names, flags, stride = list(g), _flags(g), int(g["stride"])
    P, G, nu = _unit_params(g, "1.", names, flags)
    assert nu == int(g["num_units"])
    head = next(k for k in names if k.startswith("param_0.") and k.endswith(".weight"))[len("param_"):-len(".weight")]
    for dst, pre in ((P, "param_"), (G, "grad_")):
        dst["u.in.weight"] = conv_weight_to_scn(_t(g[f"{pre}{head}.weight"]))
        dst["u.in.bias"] = _t(g[f"{pre}{head}.bias"])
    out_rows = rows_of if stride == 1 else FullGrid(g["X"].shape).coarse_rows
    return rows_of(_t(g["X"])), P, G, out_rows(_t(g["Y"])), out_rows(_t(g["dY"])), rows_of(_t(g["dX"]))


def reunite_forward(g, Xc, S, P, relu=torch.relu):
    """The decoder level of post_act_reunite.npz: coarse rows Xc (oracle order), skip rows S -> fine rows."""
    flags = _flags(g)
    fg = FullGrid(g["S"].shape)
    up = input_stage(Xc, P["u.up.weight"], P["u.up.bias"], O.swap_rules(fg.down), fg.n_fine, flags["relu_first"], False, relu)
    x = torch.cat([up, S], 1) @ P["u.nin.weight"] + P["u.nin.bias"]
    return units(x, P, "u", fg.fine_rules, fg.n_fine, num_units=int(g["num_units"]), relu=relu, **flags)


def fixture_reunite(g):
    """post_act_reunite.npz -> (coarse X rows, skip rows, P, G, Y rows, dY rows, dX rows, dS rows)."""
    names, flags = list(g), _flags(g)
    P, G, nu = _unit_params(g, "output_stage.", names, flags)
    assert nu == int(g["num_units"])
    up = next(k for k in names if k.startswith("param_input_stage.") and k.endswith(".weight"))[len("param_"):-len(".weight")]
    for dst, pre in ((P, "param_"), (G, "grad_")):
        dst["u.up.weight"] = deconv_weight_to_scn(_t(g[f"{pre}{up}.weight"]))
        dst["u.up.bias"] = _t(g[f"{pre}{up}.bias"])
        w = _t(g[f"{pre}channel_changer.weight"])                          # Conv3d 1^3 [Cout, Cin, 1, 1, 1] -> NiN [Cin, Cout]
        dst["u.nin.weight"] = w[:, :, 0, 0, 0].t().contiguous()
        dst["u.nin.bias"] = _t(g[f"{pre}channel_changer.bias"])
    fg = FullGrid(g["S"].shape)
    return (fg.coarse_rows(_t(g["X"])), rows_of(_t(g["S"])), P, G, rows_of(_t(g["Y"])), rows_of(_t(g["dY"])),
            fg.coarse_rows(_t(g["dX"])), rows_of(_t(g["dS"])))
