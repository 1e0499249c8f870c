"""A numpy float64 restatement of the class / segmentation loss path: nn.CrossEntropyLoss(weight, ignore_index,
reduction='mean') with this library's two stated deviations (a target outside [0, c) that is not ignore_index drops its row
and is counted; no valid row gives loss 0 and a zero gradient), softmax / first-index argmax, LossFilter and
ClassLossSelector's label gather in the uncompacted form (a dropped row keeps its place with the label -100)."""
import numpy as np

IGNORE = -100


def fixture_logits(z):
    """The logits of an xent_*.npz fixture: stored, or regenerated from the seed (checked against the stored checksum)."""
    if "logits" in z.files:
        return z["logits"]
    n, c, scale = int(z["n"]), int(z["c"]), float(z["scale"])
    x = (np.random.default_rng(int(z["seed"])).standard_normal((n, c)) * scale).astype(np.float32)
    assert x.astype(np.float64).sum() == float(z["checksum"]), "numpy's generator stream differs from the fixture's"
    return x


def softmax(logits):
    x = np.asarray(logits, np.float64)
    e = np.exp(x - x.max(1, keepdims=True)) if x.shape[0] else x
    return e / e.sum(1, keepdims=True) if x.shape[0] else e


def argmax_first(logits):
    x = np.asarray(logits)
    return np.argmax(x, 1).astype(np.int64) if x.shape[0] else np.zeros(0, np.int64)     # numpy: the first maximum


def cross_entropy(logits, targets, weights=None, ignore_index=IGNORE, g=1.0):
    """-> (loss, dlogits, n_bad), float64."""
    x = np.asarray(logits, np.float64)
    t = np.asarray(targets, np.int64)
    n, c = x.shape
    in_range = (t >= 0) & (t < c)
    valid = in_range & (t != ignore_index)
    n_bad = int((~in_range & (t != ignore_index)).sum())
    w_all = np.ones(c) if weights is None or len(weights) == 0 else np.asarray(weights, np.float64)
    grad = np.zeros_like(x)
    if not valid.any():
        return 0.0, grad, n_bad
    xv, tv = x[valid], t[valid]
    m = xv.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(xv - m).sum(1))
    w = w_all[tv]
    W = w.sum()
    if W == 0.0:
        return 0.0, grad, n_bad
    loss = (w * (lse - xv[np.arange(len(tv)), tv])).sum() / W
    p = np.exp(xv - lse[:, None])
    p[np.arange(len(tv)), tv] -= 1.0
    grad[valid] = g * p * (w / W)[:, None]
    return float(loss), grad, n_bad


def loss_filter(max_overlap, argmax, positive_threshold, negative_threshold=0):
    """-> (keep [P], association [P]) at the proposals' length (the reference returns association[keep])."""
    mx = np.asarray(max_overlap)
    keep = mx >= np.float32(positive_threshold)
    assoc = np.asarray(argmax, np.int64).copy()
    if negative_threshold:
        neg = mx < np.float32(negative_threshold)
        keep = keep | neg
        assoc[neg] = -1
    return keep, assoc


def select_labels(gt_association, gt_labels, negative_label=IGNORE):
    padded = np.concatenate([np.asarray(gt_labels, np.int64), [negative_label]])
    a = np.clip(np.asarray(gt_association, np.int64), -1, len(gt_labels) - 1)
    return padded[a]


def class_labels(z):
    """The uncompacted labels of a class_loss_*.npz fixture, per sample, from its overlaps / associations."""
    gt_off = np.concatenate([[0], np.cumsum(z["gt_counts"])])
    out = []
    if int(z["nodesc"]):
        p_off = np.concatenate([[0], np.cumsum(z["pred_counts"])])
        for s in range(len(z["gt_counts"])):
            sl = slice(p_off[s], p_off[s + 1])
            keep, assoc = loss_filter(z["max_overlap"][sl], z["argmax"][sl], float(z["positive_threshold"]),
                                      float(z["negative_threshold"]))
            lab = select_labels(assoc, z["gt_labels"][gt_off[s]:gt_off[s + 1]], int(z["negative_label"]))
            out.append(np.where(keep, lab, IGNORE))
    else:
        b_off = np.concatenate([[0], np.cumsum(z["box_counts"])])
        for s in range(len(z["gt_counts"])):
            out.append(select_labels(z["gt_association"][b_off[s]:b_off[s + 1]], z["gt_labels"][gt_off[s]:gt_off[s + 1]],
                                     int(z["negative_label"])))
    return out


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))
