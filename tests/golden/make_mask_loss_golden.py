"""Generates tests/golden/mask_loss_*.npz by RUNNING the reference's own mask-training path: ndsis/modules/model.py
OverlapCalculator, TrainSelector(0.2, 0, (24, 0, True)) (numpy's generator seeded right before it), the crop's inside test
(roi_select_bbox_transform.py BBoxTransformerSlice + roi_select_sparse.py get_inside_indicator, as make_roi_golden.py gets
it), SparseMaskLossSelector (the branch with a selection description) and ndsis/modules/loss.py MaskLoss, whose loss is
back-propagated to seeded mask_scores.  Run in the build container only (needs /root/reference):

    python tests/golden/make_mask_loss_golden.py

`import sparseconvnet` is satisfied by this repository's package (the classes used are pure torch).  Only inputs and
outputs are stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, "/root/reference")
import sparse_rcnn_amd                                         # noqa: E402
sys.modules["sparseconvnet"] = sparse_rcnn_amd
from ndsis.modules.model import OverlapCalculator, TrainSelector, SparseMaskLossSelector   # noqa: E402
from ndsis.modules.loss import MaskLoss                                                    # noqa: E402
from ndsis.modules.roi_select_bbox_transform import BBoxTransformerSlice                   # noqa: E402
from ndsis.modules.roi_select_sparse import get_inside_indicator                           # noqa: E402

K = 18


def boxes_near(rng, gt, n, jitter):
    """n proposals: ground-truth boxes moved and rescaled by up to `jitter` of their size (many overlap >= 0.2)."""
    if len(gt) == 0:
        return np.zeros((0, 2, 3), np.float32)
    src = gt[rng.integers(0, len(gt), size=n)].astype(np.float64)
    size = src[:, 1] - src[:, 0]
    start = src[:, 0] + rng.uniform(-jitter, jitter, (n, 3)) * size
    stop = src[:, 1] + rng.uniform(-jitter, jitter, (n, 3)) * size
    return np.stack([start, np.maximum(stop, start + 0.5)], 1).astype(np.float32)


def random_boxes(rng, n, grid, lo, hi):
    ctr = rng.uniform(0, 1, (n, 3)) * np.asarray(grid)
    edge = rng.uniform(lo, hi, (n, 3))
    return np.stack([ctr - edge / 2, ctr + edge / 2], 1).astype(np.float32)


def case(name, seed, grid, n_pts, n_gt, n_near, n_far, class_weights=False, outside_gt=False):
    rng = np.random.default_rng(seed)
    B = len(n_gt)
    coords, gts, preds, labels, masks = [], [], [], [], []
    for b in range(B):
        p = rng.integers(0, grid, size=(n_pts, 3))
        coords.append(np.concatenate([p, np.full((n_pts, 1), b)], 1))
        g = random_boxes(rng, n_gt[b], grid, 3.0, 0.7 * min(grid))
        if outside_gt and len(g):
            g[-1] = [[grid[0] + 4.25, 1.5, 1.0], [grid[0] + 9.5, 5.0, 4.0]]          # a ground truth without points
        gts.append(g)
        preds.append(np.concatenate([boxes_near(rng, g, n_near[b], 0.15), random_boxes(rng, n_far[b], grid, 2.0, 10.0)]))
        labels.append(rng.integers(0, K, size=n_gt[b]).astype(np.int64))
        masks.append(rng.uniform(0, 1, (n_gt[b], n_pts)) < 0.45)
    coords_t = torch.from_numpy(np.concatenate(coords).astype(np.int64))
    pred_t = [torch.from_numpy(p) for p in preds]
    gt_t = [torch.from_numpy(g) for g in gts]
    ov = OverlapCalculator()(pred_t, gt_t)
    np.random.seed(seed)
    fwd, descs = TrainSelector(0.2, 0, (24, 0, True))(ov)
    tr = BBoxTransformerSlice(clip=False)
    bbox_tensor, counts, assoc = tr(list(fwd), torch.tensor(grid))
    is_inside = get_inside_indicator(coords_t, bbox_tensor, assoc)
    counts = [int(c) for c in counts]
    splits = [n_pts] * B
    m = int(is_inside.sum())
    scores = torch.from_numpy((rng.normal(size=(m, K)) * 2).astype(np.float32)).requires_grad_()
    cw = torch.from_numpy(rng.uniform(0.2, 3.0, K).astype(np.float32)) if class_weights else None
    pm, gm, sl = SparseMaskLossSelector(0.2)(scores, (is_inside, counts, splits), descs, None,
                                              [torch.from_numpy(l) for l in labels], [torch.from_numpy(x) for x in masks])
    loss = MaskLoss(class_weights=cw)(pm, gm, sl)
    loss.backward()
    box_rows = is_inside.sum(1).numpy()
    out = dict(
        grid=np.array(grid, np.int64), k=np.array(K), coords=coords_t.numpy(),
        pred_boxes=np.concatenate(preds).reshape(-1, 2, 3), pred_counts=np.array([len(p) for p in preds], np.int64),
        gt_boxes=np.concatenate(gts).reshape(-1, 2, 3) if sum(n_gt) else np.zeros((0, 2, 3), np.float32),
        gt_counts=np.array(n_gt, np.int64), gt_labels=np.concatenate(labels) if sum(n_gt) else np.zeros(0, np.int64),
        gt_masks=np.packbits(np.concatenate([x.reshape(-1) for x in masks])) if sum(n_gt) else np.zeros(0, np.uint8),
        max_overlap=np.concatenate([t[2].numpy() for t in ov]), argmax=np.concatenate([t[3].numpy() for t in ov]),
        drawn=np.concatenate([d.pred_selection.numpy().astype(np.int64) for d in descs]),
        drawn_counts=np.array([len(d.pred_selection) for d in descs], np.int64),
        fwd_boxes=torch.cat(list(fwd)).numpy().reshape(-1, 2, 3), fwd_counts=np.array(counts, np.int64),
        gt_association=torch.cat([d.gt_association for d in descs]).numpy(),
        is_inside=np.packbits(is_inside.numpy(), axis=1), n_pts=np.array(n_pts), box_rows=box_rows.astype(np.int64),
        scores=scores.detach().numpy(), loss=loss.detach().numpy(), grad=scores.grad.numpy(),
        class_weights=cw.numpy() if cw is not None else np.zeros(0, np.float32))
    path = os.path.join(HERE, f"mask_loss_{name}.npz")
    np.savez_compressed(path, **out)
    npos = [int((t[2] >= 0.2).sum()) for t in ov]
    print(f"{name}: positives {npos}, drawn {out['drawn_counts'].tolist()}, boxes {counts}, rows {m}, empty boxes "
          f"{int((box_rows == 0).sum())}, loss {float(loss.detach()):.6g}, {os.path.getsize(path)} bytes")


def main():
    # more positives than 24 in sample 0, fewer in sample 1
    case("basic", 0, (40, 32, 24), 400, [6, 3], [40, 8], [10, 12])
    # class weights; three samples
    case("weights", 1, (32, 32, 16), 300, [4, 5, 2], [30, 6, 3], [4, 8, 2], class_weights=True)
    # a sample without ground truth (nothing drawn, no box), a ground truth without points (NaN, dropped)
    case("empty", 2, (32, 24, 16), 250, [4, 0, 3], [12, 0, 5], [3, 6, 2], outside_gt=True)


if __name__ == "__main__":
    main()
