"""numpy restatement of the reference's mask-training path (ndsis/modules/model.py OverlapCalculator, TrainSelector,
SparseMaskLossSelector; ndsis/modules/loss.py MaskLoss) and of the library's packed-mask layout -- the CPU side that the
fixtures (tests/golden/mask_loss_*.npz) and the device results are checked against."""
import numpy as np

f32 = np.float32


def overlap(pred, gt):
    """bbox_overlap_prediction + max(1) in fp32, every operation rounded once in the reference's order.
    pred [P, 2, 3], gt [G, 2, 3] -> (max [P] fp32, argmax [P] int64); no ground truth: 0 and 0."""
    pred, gt = np.asarray(pred, f32).reshape(-1, 2, 3), np.asarray(gt, f32).reshape(-1, 2, 3)
    P, G = len(pred), len(gt)
    if G == 0 or P == 0:
        return np.zeros(P, f32), np.zeros(P, np.int64)
    sa, ea = pred[:, None, 0], pred[:, None, 1]
    sb, eb = gt[None, :, 0], gt[None, :, 1]
    za, zb = ea - sa, eb - sb
    area_a = (za[..., 0] * za[..., 1]) * za[..., 2]
    area_b = (zb[..., 0] * zb[..., 1]) * zb[..., 2]
    e = np.maximum(np.minimum(ea, eb) - np.maximum(sa, sb), f32(0))
    inter = (e[..., 0] * e[..., 1]) * e[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        ov = inter / ((area_a + area_b) - inter)
    am = np.argmax(np.where(np.isnan(ov), np.inf, ov), 1)          # torch's max: NaN wins, the first maximum wins
    return ov[np.arange(P), am].astype(f32), am.astype(np.int64)


def inside(coords, boxes, sample):
    """The crop's rule (BBoxTransformerSlice: floor / ceil; get_inside_indicator: half open, the box's sample only):
    coords int64 [N, 4], boxes fp32 [BB, 2, 3], sample [BB] -> bool [BB, N]."""
    boxes = np.asarray(boxes, f32).reshape(-1, 2, 3)
    lo, hi = np.floor(boxes[:, 0]).astype(np.int64), np.ceil(boxes[:, 1]).astype(np.int64)
    c = np.asarray(coords)
    ok = ((c[None, :, :3] >= lo[:, None]) & (c[None, :, :3] < hi[:, None])).all(-1)
    return ok & (c[None, :, 3] == np.asarray(sample)[:, None])


def loss(scores, is_inside, box_counts, splits, assoc, labels, gt_counts, masks, class_weights=None):
    """SparseMaskLossSelector (selection-description branch) + MaskLoss in float64.
    scores [M, K] over the rows of is_inside [BB, N] (box-major, ascending point); assoc [BB] per box (-1: none); labels /
    gt_counts: concatenated per sample; masks: list of bool [G_s, N_s].  -> (loss, dscores [M, K] for an upstream 1)."""
    scores = np.asarray(scores, np.float64)
    is_inside = np.asarray(is_inside, bool)
    box_sample = np.repeat(np.arange(len(box_counts)), box_counts)
    pt_off = np.concatenate([[0], np.cumsum(splits)])
    gt_off = np.concatenate([[0], np.cumsum(gt_counts)])
    grad = np.zeros_like(scores)
    per_box, rows_of = [], []
    r0 = 0
    for b in range(is_inside.shape[0]):
        pts = np.nonzero(is_inside[b])[0]
        rows = np.arange(r0, r0 + len(pts))
        r0 += len(pts)
        s, a = box_sample[b], int(assoc[b])
        if a < 0 or a >= gt_counts[s] or len(pts) == 0:
            continue
        lab = int(labels[gt_off[s] + a])
        t = masks[s][a][pts - pt_off[s]].astype(np.float64)
        x = scores[rows, lab]
        l = np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))
        w = 1.0 if class_weights is None or len(class_weights) == 0 else float(class_weights[lab])
        per_box.append((l.mean(), w))
        rows_of.append((rows, lab, (1 / (1 + np.exp(-x)) - t) / len(pts), w))
    if not per_box:
        return 0.0, grad.astype(f32)
    W = sum(w for _, w in per_box)
    total = sum(l * w for l, w in per_box) / W
    for rows, lab, d, w in rows_of:
        grad[rows, lab] = d * w / W
    return float(total), grad.astype(f32)


def pack(mask):
    """bool [G, N] -> uint32 [G, ceil(N / 32)], bit p % 32 of word p / 32 (the library's layout)."""
    mask = np.asarray(mask, bool)
    g, n = mask.shape
    w = (n + 31) // 32
    pad = np.zeros((g, w * 32), bool)
    pad[:, :n] = mask
    bits = pad.reshape(g, w, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return bits.sum(-1).astype(np.uint32)


def unpack(words, n):
    words = np.asarray(words, np.uint32)
    bits = (words[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(words.shape[0], -1)[:, :n].astype(bool)


def fixture(z):
    """Per-sample lists of a mask_loss_*.npz: (preds, gts, labels list, masks list)."""
    pc, gc = z["pred_counts"], z["gt_counts"]
    po, go = np.concatenate([[0], np.cumsum(pc)]), np.concatenate([[0], np.cumsum(gc)])
    n = int(z["n_pts"])
    flat = np.unpackbits(z["gt_masks"])[:int(gc.sum()) * n].astype(bool) if gc.sum() else np.zeros(0, bool)
    preds = [z["pred_boxes"][po[s]:po[s + 1]] for s in range(len(pc))]
    gts = [z["gt_boxes"][go[s]:go[s + 1]] for s in range(len(gc))]
    labels = [z["gt_labels"][go[s]:go[s + 1]] for s in range(len(gc))]
    masks = [flat[go[s] * n:go[s + 1] * n].reshape(int(gc[s]), n) for s in range(len(gc))]
    return preds, gts, labels, masks


def fixture_inside(z):
    bb = int(z["fwd_counts"].sum())
    return np.unpackbits(z["is_inside"], axis=1)[:bb, :int(z["coords"].shape[0])].astype(bool)
