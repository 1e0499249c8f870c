"""Generates tests/golden/post_act_*.npz and tests/golden/post_act_keys.json by RUNNING the reference's own factory code
(ndsis/modules/module_factory.py) for the forms this package builds with relu_first=False, drop_input_relu=False and
use_residuals=False.  No source text: inputs and recorded results only.

Arrays: the dense twins the factory pairs with every scn layer, in float64 on a FULLY ACTIVE grid (2 samples, 8 x 8 x 4 at the
coarse level): with zero padding a dense same-convolution is the submanifold one, and a dense 2^3/2 (transposed) convolution is
the sparse Convolution / Deconvolution.
  post_act_unit_{plain,bottleneck}.npz   get_residual_block(3, False, C, relu_first=False): C = 16, and C = 32 at divisor 4
  post_act_level_<setting>_s<stride>.npz get_units_level(3, False, 8, 16, ...) at stride 1 and 2, for the settings of LEVELS
  post_act_reunite.npz                   get_skip_reunite_level(3, False, 16, 8, relu_first=False): Deconvolution -> ReLU
Stored: the input(s), the parameters in torch's layout (named by their state_dict keys), the output, a seeded upstream gradient
and the gradients of the input(s) and of every parameter.  Inputs, parameters and the upstream gradient are seeded draws rounded
to short dyadic numbers (inputs and parameters to halves, upstream gradients to integers), so every product and sum is exact in
float64 and the recorded results do not depend on the summation order of the machine that wrote them
(make_unit_forms_golden.py); the files hold them as integers times a power of two (`pack`).  The stride-1 files stay under
100 KB; at stride 2 the fine level has 4096 rows and its input gradient alone takes 45 KB: 100 - 165 KB per file.

get_units_level hands get_input_stage the unit switches (use_residuals, bottleneck_divisor, groups, main_path_relu), and
get_input_stage passes them on to get_activation, which does not take them: whenever an encoder level KEEPS its input ReLU
(drop_input_relu=False) the reference raises TypeError before it builds anything.  `_tolerant()` below wraps the module's
`get_activation` for exactly those calls so that it ignores the four switches -- what get_input_stage plainly means, and what
it does for a decoder level, where the switches never reach it.  Every fixture records whether it needed that (`shimmed`).

Key lists: the reference's FeatureExtractor (sparse + U-Net, plan 32-64-128-256) built ON THIS PACKAGE registered as
`sparseconvnet`, for each setting of KEYS: state_dict keys and shapes.

Run in the build container only (needs the reference's sources next to the repository):

    python tests/golden/make_post_act_golden.py
"""
import contextlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, "/root/reference")
import sparse_rcnn_amd                                         # noqa: E402
sys.modules["sparseconvnet"] = sparse_rcnn_amd
from ndsis.modules import module_factory as MF                 # noqa: E402
from ndsis.modules.model import FeatureExtractor, FeatureLevelDescriptor as FLD   # noqa: E402

LEVELS = {"pre_keep": dict(relu_first=True, drop_input_relu=False, use_residuals=True),
          "post_keep": dict(relu_first=False, drop_input_relu=False, use_residuals=True),
          "post_drop": dict(relu_first=False, drop_input_relu=True, use_residuals=True),
          "plain_pre": dict(relu_first=True, drop_input_relu=True, use_residuals=False),
          "plain_post": dict(relu_first=False, drop_input_relu=True, use_residuals=False)}
KEYS = dict(LEVELS, post_bottleneck=dict(relu_first=False, drop_input_relu=True, use_residuals=True, bottleneck_divisor=4),
            post_mainpath_keep=dict(relu_first=False, drop_input_relu=False, use_residuals=True, main_path_relu=True))
COARSE = (8, 8, 4)
SIZES = {}
UNIT_SWITCHES = ("use_residuals", "bottleneck_divisor", "groups", "main_path_relu")


@contextlib.contextmanager
def _tolerant():
    orig = MF.get_activation

    def get_activation(*a, **k):
        return orig(*a, **{n: v for n, v in k.items() if n not in UNIT_SWITCHES})
    MF.get_activation = get_activation
    try:
        yield
    finally:
        MF.get_activation = orig


def build(fn, *a, **k):
    """fn(*a, **k) -> (result, shimmed)."""
    try:
        return fn(*a, **k), False
    except TypeError as e:
        if "get_activation() got an unexpected keyword argument" not in str(e):
            raise
    with _tolerant():
        return fn(*a, **k), True


class Draw:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def __call__(self, shape, std, step):
        return torch.round(torch.randn(tuple(shape), generator=self.g, dtype=torch.float64) * std / step) * step


def pack(out):
    """Every array is a short dyadic number times an integer: store the integers in the narrowest type and the step beside them
    (`<name>__step`; tests/post_act_restate.load multiplies them out, exactly)."""
    packed = {}
    for k, a in out.items():
        a = np.asarray(a)
        if a.dtype != np.float64 or a.ndim == 0:
            packed[k] = a
            continue
        step = 1.0
        while not np.array_equal(np.round(a / step), a / step):
            step /= 2
            assert step > 2.0 ** -40, k
        q = np.round(a / step).astype(np.int64)
        t = next(t for t in (np.int8, np.int16, np.int32, np.int64) if np.abs(q).max(initial=0) <= np.iinfo(t).max)
        assert np.array_equal(q.astype(t).astype(np.float64) * step, a)
        packed[k], packed[k + "__step"] = q.astype(t), np.array(step)
    return packed


def record(name, layer, inputs, draw, extra):
    layer = layer.double()
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(draw(p.shape, 0.4, 0.5))
    xs = [x.requires_grad_() for x in inputs.values()]
    Y = layer(*[x.clone() for x in xs])                        # (the dense activations work in place)
    dY = draw(Y.shape, 1.0, 1.0)
    params = list(layer.parameters())
    grads = torch.autograd.grad(Y, xs + params, dY)
    out = dict(Y=Y.detach().numpy(), dY=dY.numpy(), **{k: np.array(v) for k, v in extra.items()})
    for (k, x), gx in zip(inputs.items(), grads):
        out[k], out["d" + k] = x.detach().numpy(), gx.numpy()
    for (pn, p), gp in zip(layer.named_parameters(), grads[len(xs):]):
        out["param_" + pn] = p.detach().numpy()
        out["grad_" + pn] = gp.numpy()
    path = os.path.join(HERE, f"post_act_{name}.npz")
    np.savez_compressed(path, **pack(out))
    print(name, [k for k in out if k.startswith("param_")], os.path.getsize(path), "bytes")
    SIZES[name] = os.path.getsize(path)


def switches(relu_first=True, drop_input_relu=True, use_residuals=True, bottleneck_divisor=0, main_path_relu=False):
    return dict(relu_first=relu_first, drop_input_relu=drop_input_relu, use_residuals=use_residuals,
                bottleneck_divisor=bottleneck_divisor, main_path_relu=main_path_relu)


def unit_arrays(name, C, divisor, seed):
    (sp, stride, ch, layer), shim = build(MF.get_residual_block, 3, False, C, relu_first=False, batchnorm=False,
                                          bottleneck_divisor=divisor, main_path_relu=False)
    assert not sp and ch == C
    draw = Draw(seed)
    record(f"unit_{name}", layer, dict(X=draw((2, C) + COARSE, 1.0, 0.5)), draw,
           dict(switches(relu_first=False, bottleneck_divisor=divisor), shimmed=shim))


def level_arrays(name, flags, stride, seed, cin=8, cout=16):
    num_units = 1 if flags["use_residuals"] else 2
    (sp, _, ch, layer), shim = build(MF.get_units_level, 3, False, cin, cout, num_units=num_units, make_dense=False, stride=stride,
                                     batchnorm=False, bottleneck_divisor=0, groups=1, main_path_relu=False, **flags)
    assert not sp and ch == cout
    draw = Draw(seed)
    fine = tuple(s * stride for s in COARSE)
    record(f"level_{name}_s{stride}", layer, dict(X=draw((2, cin) + fine, 1.0, 0.5)), draw,
           dict(switches(**flags), stride=stride, num_units=num_units, shimmed=shim))


def reunite_arrays(seed, cin=16, cskip=8):
    (sp, _, ch, layer), shim = build(MF.get_skip_reunite_level, 3, False, cin, cskip, stride=2, use_residuals=True, bottleneck_divisor=0,
                                     main_path_relu=False, num_units=1, relu_first=False, batchnorm=False)
    assert not sp and ch == cskip
    draw = Draw(seed)
    fine = tuple(s * 2 for s in COARSE)
    record("reunite", layer, dict(X=draw((2, cin) + COARSE, 1.0, 0.5), S=draw((2, cskip) + fine, 1.0, 0.5)), draw,
           dict(switches(relu_first=False), num_units=1, shimmed=shim))


def feature_extractor(channels, flags, cin=7):
    """make_unit_forms_golden.feature_extractor with every switch; each level takes the network's drop_input_relu."""
    f = switches(**flags)
    layer_descriptions = [FLD('B', channels[0], dict(stride=1)), *[FLD('B', c) for c in channels[1:]]]
    unit = dict(use_residuals=f["use_residuals"], relu_first=f["relu_first"], bottleneck_divisor=f["bottleneck_divisor"],
                main_path_relu=f["main_path_relu"], batchnorm=False, num_units=2)
    unet_params = dict(groups=1, concat=True, min_channels=16, **unit)
    params = dict(num_dims=3, sparse=True, input_channels=cin, network_description=layer_descriptions,
                  class_output_anchor=False, class_output_upsampled=False, class_output_index=-1, num_dilations=5,
                  stride=2, maxpool=False, bottleneck_groups=1, drop_input_relu=f["drop_input_relu"], include_unet=True,
                  unet_params=unet_params, **unit)
    return build(FeatureExtractor, **params)


if __name__ == "__main__":
    unit_arrays("plain", 16, 0, 60)
    unit_arrays("bottleneck", 32, 4, 61)
    for k, (name, flags) in enumerate(LEVELS.items()):
        for stride in (1, 2):
            level_arrays(name, flags, stride, 70 + 2 * k + stride)
    reunite_arrays(90)
    keys = {}
    channels = [32, 64, 128, 256]
    for name, flags in KEYS.items():
        fx, shim = feature_extractor(channels, flags)
        sd = fx.state_dict()
        keys[name] = dict(channels=channels, flags=switches(**flags), shimmed=shim,
                          n_params=int(sum(v.numel() for v in sd.values())), keys={k: list(v.shape) for k, v in sd.items()})
        print(name, keys[name]["n_params"], len(sd), "shimmed" if shim else "")
    with open(os.path.join(HERE, "post_act_keys.json"), "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
    assert max(SIZES.values()) < 200_000, SIZES
