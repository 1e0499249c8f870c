"""Generates tests/golden/unit_form_{bottleneck,mainpath,both}.npz and tests/golden/unit_forms_keys.json by RUNNING the
reference's own factory code (ndsis/modules/module_factory.py:127-183 `get_residual_block`, relu_first=True) for the three unit
forms this package adds to the plain pre-activation unit: bottleneck_divisor=4, main_path_relu=True, and both.

Arrays: `get_residual_block(3, sparse=False, 16, ...)` -- the dense twin the factory pairs with every scn layer -- in float64 on
a FULLY ACTIVE grid [2, 16, 5, 4, 3]: with zero padding that is the submanifold case (every cell is an active site, no bias
leaks into an inactive one), as make_dense_twin_golden.py uses for batch norm.  Stored: the input, the parameters in torch's
layout (named by their state_dict keys), the output, a seeded upstream gradient and the gradients of the input and of every
parameter.  No source text: inputs and recorded results only.  Inputs, parameters and the upstream gradient are seeded normal
draws rounded to multiples of 1/4 (input, gradient) and 1/8 (parameters): every product and sum of the unit is then exact in
float64 (< 40 significant bits), so the recorded results do not depend on the summation order of the machine that wrote them,
and their low mantissa bytes are zero, which keeps the 2 x 27 x 16 x 16 float64 weight gradients of the main-path form under
100 KB compressed.

Key lists: the reference's FeatureExtractor (sparse + U-Net, plan 32-64-128-256) built ON THIS PACKAGE registered as
`sparseconvnet` with each switch combination, as make_dropin_golden.py does for the default form: state_dict keys and shapes.

Run in the build container only (needs the reference's sources next to the repository):

    python tests/golden/make_unit_forms_golden.py
"""
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

FORMS = {"bottleneck": dict(bottleneck_divisor=4, main_path_relu=False),
         "mainpath": dict(bottleneck_divisor=0, main_path_relu=True),
         "both": dict(bottleneck_divisor=4, main_path_relu=True)}
C, SHAPE = 16, (2, 16, 5, 4, 3)


def unit_arrays(name, flags, seed):
    sp, stride, ch, layer = MF.get_residual_block(3, False, C, relu_first=True, batchnorm=False, **flags)
    assert not sp and ch == C
    layer = layer.double()
    g = torch.Generator().manual_seed(seed)

    def draw(shape, std, step):
        return torch.round(torch.randn(shape, generator=g, dtype=torch.float64) * std / step) * step
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(draw(p.shape, 0.3, 0.125))
    X = draw(SHAPE, 1.0, 0.25).requires_grad_()
    Y = layer(X)
    dY = draw(Y.shape, 1.0, 0.25)
    params = list(layer.parameters())
    grads = torch.autograd.grad(Y, [X] + params, dY)
    out = dict(X=X.detach().numpy(), Y=Y.detach().numpy(), dY=dY.numpy(), dX=grads[0].numpy(),
               bottleneck_divisor=np.array(flags["bottleneck_divisor"]), main_path_relu=np.array(flags["main_path_relu"]))
    for (pn, p), gp in zip(layer.named_parameters(), grads[1:]):
        out["param_" + pn] = p.detach().numpy()
        out["grad_" + pn] = gp.numpy()
    path = os.path.join(HERE, f"unit_form_{name}.npz")
    np.savez_compressed(path, **out)
    print(name, type(layer).__name__, [k for k in out if k.startswith("param_")], os.path.getsize(path), "bytes")


def feature_extractor(channels, flags, cin=7):
    """make_dropin_golden.build with the two switches passed where scannet_config/run.py passes them (:516-518, 609-620)."""
    layer_descriptions = [FLD('B', channels[0], dict(stride=1, drop_input_relu=True)), *[FLD('B', c) for c in channels[1:]]]
    unet_params = dict(use_residuals=True, num_units=2, groups=1, relu_first=True, batchnorm=False, concat=True, min_channels=16,
                       **flags)
    params = dict(num_dims=3, sparse=True, input_channels=cin, network_description=layer_descriptions,
                  class_output_anchor=False, class_output_upsampled=False, class_output_index=-1, num_dilations=5,
                  num_units=2, stride=2, maxpool=False, relu_first=True, bottleneck_groups=1, batchnorm=False,
                  use_residuals=True, drop_input_relu=True, include_unet=True, unet_params=unet_params, **flags)
    return FeatureExtractor(**params)


if __name__ == "__main__":
    for k, (name, flags) in enumerate(FORMS.items()):
        unit_arrays(name, flags, 40 + k)
    keys = {}
    channels = [32, 64, 128, 256]
    for name, flags in FORMS.items():
        sd = feature_extractor(channels, flags).state_dict()
        keys[name] = dict(channels=channels, flags=flags, n_params=int(sum(v.numel() for v in sd.values())),
                          keys={k: list(v.shape) for k, v in sd.items()})
        print(name, keys[name]["n_params"], len(sd))
    with open(os.path.join(HERE, "unit_forms_keys.json"), "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
