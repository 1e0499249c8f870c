"""Generates tests/golden/anchor_up_*.npz and anchor_up_keys.json by RUNNING the reference's own up-sampling RPN heads
(ndsis/modules/anchor_network.py:127-219 AnchorNetworkUpsample: one ConvTranspose3d per group of anchors, AnchorStorage's
anchors and inside indicator, `rpn_permuter` + `rpn_bbox_score_splitter`) on the CPU, forward and backward, on seeded volumes
with the reference's own extra strides and groups (scannet_config/network.py:24-41).  Needs a checkout of the reference
(LeonhardFeiner/sparse_rcnn); nothing of it is copied, only what its code computes is stored:

    SPARSE_RCNN_REFERENCE=<checkout> python tests/golden/make_anchor_up_golden.py

Anchor sizes are the reference's in voxels times a scale, so that small scenes hold inside anchors.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
if not os.environ.get("SPARSE_RCNN_REFERENCE"):
    raise SystemExit("set SPARSE_RCNN_REFERENCE to a checkout of the reference")
sys.path.insert(0, os.environ["SPARSE_RCNN_REFERENCE"])
import sparse_rcnn_amd                                         # noqa: E402
sys.modules["sparseconvnet"] = sparse_rcnn_amd
if not hasattr(np, "int"):
    np.int = int                 # scannet_config/network.py predates the alias's removal; it imports nothing but numpy
from scannet_config import network as N                        # noqa: E402
from ndsis.modules.anchor_network import AnchorNetworkUpsample  # noqa: E402

VOXEL_M = 0.0375                 # scannet_config/run.py:361-362
CONV_STRIDES = (4, 8)


def build(scale, channels, border):
    anchors = [[np.asarray(a) / VOXEL_M * scale for a in lv] for lv in N.calculated_anchor_levels]     # run.py:830-833
    net = AnchorNetworkUpsample(anchors, [np.full(3, s) for s in CONV_STRIDES], channels, border,
                                extra_stride_levels=N.calculated_stride_levels)
    return net, anchors


def case(name, seed, scene_shape, scale, border, batch, channels=(8, 8)):
    torch.manual_seed(seed)
    net, anchors = build(scale, channels, border)
    g = torch.Generator().manual_seed(seed + 100)
    sizes = [tuple(v // s for v in scene_shape) for s in CONV_STRIDES]
    feats = [torch.randn((batch, c) + sz, generator=g).requires_grad_() for c, sz in zip(channels, sizes)]
    bbox, score, desc = net(feats, tuple(scene_shape))
    g_bbox = torch.randn(bbox.shape, generator=g)
    g_score = torch.randn(score.shape, generator=g)
    torch.autograd.backward([bbox, score], [g_bbox, g_score])
    out = dict(scene_shape=np.array(scene_shape, np.int64), conv_strides=np.array(CONV_STRIDES, np.int64),
               border=np.array(border), batch=np.array(batch), n_levels=np.array(len(feats)),
               inside_indicator=desc.inside_indicator.numpy(), inside_anchors=desc.inside_anchors.numpy(),
               rpn_bbox=bbox.detach().numpy(), rpn_score=score.detach().numpy(), g_bbox=g_bbox.numpy(), g_score=g_score.numpy())
    for l, f in enumerate(feats):
        heads = list(net.rpn_net_levels.operation[l])
        out[f"feat{l}"] = f.detach().numpy()
        out[f"dfeat{l}"] = f.grad.numpy()
        out[f"n_groups{l}"] = np.array(len(heads))
        out[f"extra_strides{l}"] = np.asarray(N.calculated_stride_levels[l], np.int64)
        for k, h in enumerate(heads):
            out[f"anchors{l}_{k}"] = np.asarray(anchors[l][k], np.float64)
            out[f"w{l}_{k}"] = h.weight.detach().numpy()
            out[f"b{l}_{k}"] = h.bias.detach().numpy()
            out[f"dw{l}_{k}"] = h.weight.grad.numpy()
            out[f"db{l}_{k}"] = h.bias.grad.numpy()
    np.savez_compressed(os.path.join(HERE, f"anchor_up_{name}.npz"), **out)
    ins = desc.inside_indicator
    per_group, o = [], 0
    for l, sz in enumerate(sizes):
        for k, e in enumerate(N.calculated_stride_levels[l]):
            n = int(np.prod(sz) * np.prod(e) * len(anchors[l][k]))
            per_group.append(int(ins[o:o + n].sum()))
            o += n
    print(name, "anchors", len(ins), "inside", int(ins.sum()), "per group", per_group)


def keys():
    net, anchors = build(1.0, (128, 256), 0)
    sd = net.state_dict()
    doc = dict(keys={k: list(v.shape) for k, v in sd.items()},
               learned=[k for k, _ in net.named_parameters() if k.startswith("rpn_net_levels.")],
               extra_stride_levels=[np.asarray(s).tolist() for s in N.calculated_stride_levels],
               anchor_levels_voxels=[[np.asarray(a).tolist() for a in lv] for lv in anchors])
    with open(os.path.join(HERE, "anchor_up_keys.json"), "w") as f:
        json.dump(doc, f, indent=1)
    print("keys", len(doc["keys"]), "learned", len(doc["learned"]))


if __name__ == "__main__":
    case("all_inside", 0, (24, 16, 8), 0.12, 0, 2)
    case("mixed", 1, (40, 24, 16), 0.25, 0, 3)
    case("border", 2, (24, 16, 8), 0.25, 3, 1)
    keys()
