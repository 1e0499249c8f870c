"""Torch restatement of the reference's RESHAPING class head (`simple_class`, scannet_config/run.py:706-710), written from its
description: identity input network, RoiAlign (tests/roialign_restate.py), max_pool3d(2), one bare 3^3
same-convolution per level (no ReLU before or between them), the channel-major flatten `x.view(R, -1)` of [R, C, x, y, z], then
ReLU Linear ReLU Linear.  Works on CPU and device tensors, fp32 or fp64; autograd gives the gradients.
tests/test_reshape_class_cpu.py checks it against the fixtures the reference's own code produced."""
import torch.nn.functional as TF

import roialign_restate as R


def n_same_levels(sd):
    n = 0
    while f"output_conv_layer.{n + 1}.weight" in sd:
        n += 1
    return n


def reshape_class_forward(sd, volume_ncxyz, bbox_batch, stride, cut_shape=(8, 8, 8)):
    """The head from the reference's state dict `sd` (its own keys, nn.Conv3d / nn.Linear layouts), in eval mode.
    -> (class scores [R, classes], bbox_tensor, counts)."""
    size = volume_ncxyz.shape[2:]
    bbox_tensor, counts, sample = R.transform_boxes(bbox_batch, size, stride, True)
    cut = R.roialign(volume_ncxyz.permute(0, 2, 3, 4, 1), bbox_tensor.to(volume_ncxyz.device), sample, cut_shape)
    x = TF.max_pool3d(cut.permute(0, 4, 1, 2, 3), 2)
    for l in range(1, n_same_levels(sd) + 1):
        x = TF.conv3d(x, sd[f"output_conv_layer.{l}.weight"], sd[f"output_conv_layer.{l}.bias"], padding=1)
    x = x.reshape(x.shape[0], -1)                              # channel-major: column (c X + x) Y Z + y Z + z
    x = TF.linear(TF.relu(x), sd["linear_layer.1.weight"], sd["linear_layer.1.bias"])
    x = TF.linear(TF.relu(x), sd["linear_layer.3.weight"], sd["linear_layer.3.bias"])
    return x, bbox_tensor, counts


def load_fixture(golden_dir, name):
    """reshape_class_<name>.npz / .json with the seeded inputs regenerated -> dict: numpy arrays of the .npz plus `keys`,
    `params` {reference key: fp32 array}, `volume` [B, X, Y, Z, C], `bbox_batch` (list per sample), `_size`, `_batch`, `_c`."""
    import json
    import os
    import numpy as np
    z = dict(np.load(os.path.join(golden_dir, f"reshape_class_{name}.npz")))
    meta = json.load(open(os.path.join(golden_dir, f"reshape_class_{name}.json")))
    seed, batch, size, c = int(z["seed"]), int(z["batch"]), tuple(int(v) for v in z["size"]), int(z["c"])
    z["keys"], z["same_channels"] = meta["keys"], meta["same_channels"]
    z["params"] = R.seeded_params(meta["keys"], seed)
    z["volume"] = R.seeded_volume(seed, batch, size, c)
    cs = R.checksum(z["volume"], z["score_grad"], *[z["params"][k] for k in sorted(z["params"])])
    assert abs(cs - float(z["checksum"])) <= 1e-9 * max(1.0, abs(float(z["checksum"])))
    counts, o, boxes = [int(v) for v in z["counts"]], 0, []
    for n in counts:
        boxes.append(z["boxes"][o:o + n])
        o += n
    z["bbox_batch"], z["_size"], z["_batch"], z["_c"] = boxes, size, batch, c
    return z
