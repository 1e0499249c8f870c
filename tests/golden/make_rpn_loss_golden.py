"""Generates tests/golden/rpn_loss_*.npz by RUNNING the reference's own RPN loss: ndsis/modules/anchor.py
AnchorDescriptionMultiLevel (inside anchors, `get_bbox_targets` = select_bbox + bbox_transform), ndsis/modules/loss.py
BatchwiseBboxTargetSelector(0.35, 0.15, 1/8) (numpy's generator seeded right before it) and RpnLoss(sigma=2), whose summed loss
is back-propagated to seeded rpn_score / rpn_bbox.  Run in the build container only (needs /root/reference):

    python tests/golden/make_rpn_loss_golden.py
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, "/root/reference")
import sparse_rcnn_amd                                         # noqa: E402
sys.modules["sparseconvnet"] = sparse_rcnn_amd
from ndsis.modules.anchor import AnchorDescriptionMultiLevel   # noqa: E402
from ndsis.modules.loss import BatchwiseBboxTargetSelector, RpnLoss   # noqa: E402
from sparse_rcnn_amd import rpn as R                           # noqa: E402  (anchor tables only)


class _Capture(nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.out = inner, None

    def forward(self, *a):
        self.out = self.inner(*a)
        return self.out


def boxes(g, n, scene, lo, hi):
    scene = torch.tensor(scene, dtype=torch.float32)
    ctr = torch.rand((n, 3), generator=g) * scene
    edge = lo + torch.rand((n, 3), generator=g) * (hi - lo)
    start = ctr - edge / 2
    return torch.stack([start, start + edge], 1)


def case(name, seed, scene_shape, conv_shapes, strides, anchor_levels, gt_bbox):
    g = torch.Generator().manual_seed(seed)
    raw_levels = [torch.tensor(a, dtype=torch.float32) for a in anchor_levels]
    stride_levels = torch.tensor([[float(s)] * 3 for s in strides])
    desc = AnchorDescriptionMultiLevel(tuple(scene_shape), [tuple(c) for c in conv_shapes], raw_levels, stride_levels)
    n, batch = len(desc.inside_anchors), len(gt_bbox)
    calc = _Capture(lambda gt: desc.get_bbox_targets(gt))
    sel = _Capture(BatchwiseBboxTargetSelector(0.35, 0.15, max_weight=1 / 8))
    loss = RpnLoss(sel, 2.)
    rpn_score = (torch.randn((batch, n), generator=g) * 2).requires_grad_()
    rpn_bbox = (torch.randn((batch, n, 2, 3), generator=g) * 0.4).requires_grad_()
    np.random.seed(seed)
    score_loss, bbox_loss = loss(gt_bbox, calc, rpn_score, rpn_bbox)
    (score_loss + bbox_loss).backward()
    ov, am, tg = calc.out
    labels, sw, bw = sel.out
    offs = np.cumsum([0] + [len(b) for b in gt_bbox]).astype(np.int64)
    out = dict(scene_shape=np.array(scene_shape, np.int64), strides=np.array(strides, np.int64),
               inside_anchors=desc.inside_anchors.numpy(), gt_boxes=torch.cat(gt_bbox).numpy().reshape(-1, 2, 3),
               gt_offsets=offs, max_overlaps=ov.numpy(), argmax=am.numpy(), bbox_targets=tg.numpy(),
               labels=labels.numpy(), score_weight=sw.numpy(), bbox_weights=bw.numpy(),
               rpn_score=rpn_score.detach().numpy(), rpn_bbox=rpn_bbox.detach().numpy(),
               score_loss=score_loss.detach().numpy(), bbox_loss=bbox_loss.detach().numpy(),
               grad_score=rpn_score.grad.numpy(), grad_bbox=rpn_bbox.grad.numpy(), n_levels=np.array(len(anchor_levels)))
    for l, (a, c) in enumerate(zip(anchor_levels, conv_shapes)):
        out[f"anchors{l}"] = np.array(a, np.float32)
        out[f"conv_shape{l}"] = np.array(c, np.int64)
    path = os.path.join(HERE, f"rpn_loss_{name}.npz")
    np.savez_compressed(path, **out)
    pos, neg = int((ov >= 0.35).sum()), int((ov < 0.15).sum())
    print(f"{name}: {batch} x {n} anchors, boxes {offs.tolist()}, pos {pos} neg {neg}, losses {float(score_loss.detach()):.6g} "
          f"{float(bbox_loss.detach()):.6g}, {os.path.getsize(path)} bytes")


def main():
    g = torch.Generator().manual_seed(7)
    # one level, the stand-in's anchor table
    case("one_level", 0, (64, 48, 32), [(8, 6, 4)], [8], [R.DEFAULT_ANCHORS],
         [boxes(g, 7, (64, 48, 32), 8, 40), boxes(g, 12, (64, 48, 32), 6, 50)])
    # the reference's two anchor levels (stride 4: 3 anchors, stride 8: 11 anchors)
    case("two_levels", 1, (32, 32, 24), [(8, 8, 6), (4, 4, 3)], [4, 8], R.REF_ANCHOR_LEVELS_VOXELS,
         [boxes(g, 9, (32, 32, 24), 6, 30), boxes(g, 5, (32, 32, 24), 8, 28)])
    # the middle sample has no boxes: overlap 0, argmax -1, zero matched box
    case("empty_sample", 2, (48, 48, 32), [(6, 6, 4)], [8], [R.DEFAULT_ANCHORS[:3]],
         [boxes(g, 6, (48, 48, 32), 8, 40), torch.zeros((0, 2, 3)), boxes(g, 3, (48, 48, 32), 10, 30)])
    # a small scene with large boxes: more positives than negatives (the positives are drawn)
    cells = [(x, y, z) for x in (12, 20) for y in (12, 20) for z in (12, 20)][2:]
    b = torch.tensor([[[x - 7 + 0.3, y - 7, z - 7.2], [x + 7.3, y + 7, z + 6.9]] for x, y, z in cells], dtype=torch.float32)
    case("pos_gt_neg", 3, (32, 32, 32), [(4, 4, 4)], [8], [((12.0, 12.0, 12.0), (16.0, 16.0, 16.0))], [b, b[:4] + 1.0])
    # positives only: min_count 0, every score weight 0
    case("no_negatives", 3, (24, 24, 24), [(3, 3, 3)], [8], [((16.0, 16.0, 16.0), (20.0, 20.0, 20.0))],
         [torch.tensor([[[0.5, 0.5, 0.5], [23.0, 23.5, 22.0]], [[1.0, 2.0, 0.0], [20.0, 24.0, 21.0]]]),
          torch.tensor([[[2.0, 0.0, 1.0], [24.0, 22.0, 24.0]]])])
    # equal counts: four boxes equal to four anchors (IoU 1), the four other anchors only touch them (IoU 0)
    a = [[(x * 8 + 4.0 - 4, y * 8 + 4.0 - 4, z * 8 + 4.0 - 4), (x * 8 + 4.0 + 4, y * 8 + 4.0 + 4, z * 8 + 4.0 + 4)]
         for x, y, z in ((0, 0, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1))]
    case("pos_eq_neg", 4, (16, 16, 16), [(2, 2, 2)], [8], [((8.0, 8.0, 8.0),)], [torch.tensor(a, dtype=torch.float32)])


if __name__ == "__main__":
    main()
