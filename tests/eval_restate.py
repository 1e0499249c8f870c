"""Restatement of the reference's evaluation (ndsis/training/evaluation.py, ndsis/utils/mask.py:62-148, bbox.py
bbox_overlap_prediction) in numpy: integer counts, the sequential matching, a float64 curve.  tests/test_evaluation_cpu.py
pins it to the fixtures the reference wrote (tests/golden/eval_*.npz); the at-size GPU tests then check the device against
it, since the reference does not travel with the repository.

Exact by construction: intersections and unions are integer matrix products; an IoU is ONE fp32 division of two exactly
represented integers (numpy rounds it correctly, as torch and the device do); the box IoU is fp32 numpy in the reference's
operation order, one rounding per operation.  The curve is float64: the device's fp32 curve is compared within n * 2^-24."""
import warnings

import numpy as np

EPS24 = 2.0 ** -24


def ap_bound(n_points):
    """AP / mAP / mean IoU: only the order of a final fp32 sum of n terms that total <= 1 can differ."""
    return max(int(n_points), 1) * EPS24


def nanmean(a):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        return np.nanmean(a)


def unpack_rows(packed, rows, n):
    """np.packbits(bool [rows, n], axis=1) -> bool [rows, n]."""
    if rows == 0 or n == 0:
        return np.zeros((rows, n), bool)
    return np.unpackbits(np.asarray(packed, np.uint8).reshape(rows, -1), axis=1)[:, :n].astype(bool)


def words_of(mask):
    """bool [rows, n] -> uint32 [rows, ceil(n / 32)], bit p % 32 of word p / 32 = column p (the device's packed layout)."""
    rows, n = mask.shape
    w = (n + 31) // 32
    m = np.zeros((rows, w * 32), np.uint8)
    m[:, :n] = mask
    return np.packbits(m.reshape(rows, w, 4, 8), axis=-1, bitorder="little").reshape(rows, w, 4).copy().view("<u4").reshape(rows, w)


def mask_counts(pred, gt):
    """bool [P, N], bool [G, N] -> inter int64 [P, G], |pred| [P], |gt| [G]."""
    assert pred.shape[1] < (1 << 24)                          # fp32 sums of ones are exact below 2^24
    inter = np.rint(pred.astype(np.float32) @ gt.astype(np.float32).T).astype(np.int64)
    return inter, pred.sum(1).astype(np.int64), gt.sum(1).astype(np.int64)


def iou_from_counts(inter, pc, gc):
    union = pc[:, None] + gc[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter.astype(np.float32) / union.astype(np.float32)


def mask_iou(pred, gt):
    return iou_from_counts(*mask_counts(pred, gt))


def pair_confusion(pred, gt):
    """mask_confusion_pair of row i against row i: int64 [G, 2, 2] = [[tp, fp], [fn, tn]]."""
    n = pred.shape[1]
    tp = (pred & gt).sum(1).astype(np.int64)
    pc, gc = pred.sum(1).astype(np.int64), gt.sum(1).astype(np.int64)
    return np.stack([np.stack([tp, pc - tp], -1), np.stack([gc - tp, n - (pc + gc - tp)], -1)], -2)


def box_iou(pred, gt):
    """fp32 [P, 2, 3] x [G, 2, 3] -> fp32 [P, G], bbox_overlap_prediction's operation order."""
    a, b = np.asarray(pred, np.float32)[:, None], np.asarray(gt, np.float32)[None]
    sa, sb = a[..., 1, :] - a[..., 0, :], b[..., 1, :] - b[..., 0, :]
    va, vb = (sa[..., 0] * sa[..., 1]) * sa[..., 2], (sb[..., 0] * sb[..., 1]) * sb[..., 2]
    e = np.maximum(np.minimum(a[..., 1, :], b[..., 1, :]) - np.maximum(a[..., 0, :], b[..., 0, :]), np.float32(0))
    inter = (e[..., 0] * e[..., 1]) * e[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (inter / ((va + vb) - inter)).astype(np.float32)


def match(iou, threshold):
    """calc_tp_indicator (evaluation.py:619-649): walk the predictions in order; the maximum over the ground truths not yet
    matched, the first index on a tie, a NaN among them wins (torch's max) and fails `>= threshold`."""
    p, g = iou.shape
    tp = np.zeros(p, bool)
    remaining = list(range(g))
    thr = np.float32(threshold)                              # the comparison is an fp32 one
    for i in range(p):
        if not remaining:
            break
        row = iou[i, remaining]
        if np.isnan(row).any():
            continue
        j = int(np.argmax(row))                              # first maximum
        if row[j] >= thr:
            remaining.pop(j)
            tp[i] = True
    return tp


def problem(rec, threshold, cls=None):
    """One sample's record dict(score, iou, keep, pred_class, gt_class) -> (scores of its predictions, tp flags, num_gt)."""
    keep = np.ones(len(rec["score"]), bool) if rec.get("keep") is None else np.asarray(rec["keep"], bool)
    cols = np.ones(rec["iou"].shape[1], bool)
    if cls is not None:
        keep = keep & (np.asarray(rec["pred_class"]) == cls)
        cols = np.asarray(rec["gt_class"]) == cls
    return rec["score"][keep], match(rec["iou"][keep][:, cols], threshold), int(cols.sum())


class Curve:
    """PrecisionRecallCurve in float64 over a data set's records; stable descending sort (this package's tie rule)."""

    def __init__(self, records, threshold, cls=None):
        parts = [problem(r, threshold, cls) for r in records]
        score = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.float32)
        tp = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, bool)
        self.num_gt = sum(p[2] for p in parts)
        order = np.argsort(-score.astype(np.float64), kind="stable")
        self.score, self.tp_indicator = score[order], tp[order]
        c = np.cumsum(self.tp_indicator.astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            self.precision = c / np.arange(1, len(c) + 1)
            self.recall = c / self.num_gt
        self.precision_interpolated = np.maximum.accumulate(self.precision[::-1])[::-1] if len(c) else self.precision

    def ap(self, method=None):
        if method is None:
            if len(self.recall):
                return float(((self.recall - np.concatenate([[0.0], self.recall[:-1]])) * self.precision_interpolated).sum())
            return 0.0 if self.num_gt else float("nan")
        if not self.num_gt:
            return float("nan")
        samples = np.linspace(0, 1, method, dtype=np.float32).astype(np.float64)      # torch.linspace in fp32
        rec32 = self.recall.astype(np.float32).astype(np.float64)                      # `recall > samples` is an fp32 compare
        out = []
        for s in samples:
            idx = np.nonzero(rec32 > s)[0]
            out.append(self.precision_interpolated[idx[0]] if len(idx) else 0.0)
        return float(np.mean(out))


def confusion(pred, gt, c):
    pred, gt = np.asarray(pred, np.int64), np.asarray(gt, np.int64)
    v = (gt >= 0) & (gt < c)
    assert ((pred[v] >= 0) & (pred[v] < c)).all()
    return np.bincount(pred[v] * c + gt[v], minlength=c * c).reshape(c, c).astype(np.int64)


def confusion_iou(m):
    tp = np.diag(m)
    union = m.sum(1) + m.sum(0) - tp
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = tp.astype(np.float32) / union.astype(np.float32)
    return iou, nanmean(iou)


def binary_collection(conf, labels, classes):
    """BinaryConfusionMatrixCollection: -> (classwise matrices [2, 2, C], classwise_iou, average_iou, classwise_mean_iou,
    mean_average_iou)."""
    conf, labels = np.asarray(conf, np.int64).reshape(-1, 2, 2), np.asarray(labels)
    mats, mean_iou = [], []
    for c in classes:
        t = conf[labels == c]
        mats.append(t.sum(0))
        with np.errstate(divide="ignore", invalid="ignore"):
            i = t[:, 0, 0].astype(np.float32) / (t[:, 0, 0] + t[:, 0, 1] + t[:, 1, 0]).astype(np.float32)
        mean_iou.append(float(i.astype(np.float64).mean()) if len(i) else float("nan"))
    mats = np.stack(mats, -1)
    tp, union = mats[0, 0], mats[0, 0] + mats[0, 1] + mats[1, 0]
    iou = np.array([a / u if u else float("nan") for a, u in zip(tp, union)])
    return mats, iou, nanmean(iou), np.array(mean_iou), nanmean(mean_iou)


def name_of(name, metric, threshold, method):
    return f"{name}_{metric}_{threshold}" + ("" if method is None else "_{method}_points")


def metrics(overlaps, confusions, overlap_confusions, binaries, thresholds, class_indices, class_names, methods=(None, 11),
            confusion_names=None):
    """EvaluationHelper.__call__: overlaps {name: list of records}, confusions / overlap_confusions {name: int64 [C, C]},
    binaries {name: (conf [n, 2, 2], labels [n])} -> (combined, single_class, n_curve_points {name: largest curve})."""
    single = [t for t in thresholds if not isinstance(t, tuple)]
    multi = [t for t in thresholds if isinstance(t, tuple)]
    all_thr = sorted({*single, *(t for _, ts in multi for t in ts)})
    combined, single_class, n_points = {}, {}, {}
    for name, recs in overlaps.items():
        has_classes = all(r.get("pred_class") is not None for r in recs)
        ap, cap = {}, {}
        for t in all_thr:
            cur = Curve(recs, t)
            n_points[name] = max(n_points.get(name, 1), len(cur.recall))
            cols = [Curve(recs, t, c) for c in class_indices] if has_classes else []
            for m in methods:
                ap[t, m] = cur.ap(m)
                if has_classes:
                    cap[t, m] = np.array([c.ap(m) for c in cols])
        for m in methods:
            for t in single:
                combined[name_of(name, "AP", t, m)] = ap[t, m]
                if has_classes:
                    combined[name_of(name, "mAP", t, m)] = nanmean(cap[t, m])
                    single_class[name_of(name, "class_AP", t, m)] = {class_names[i]: v for i, v in enumerate(cap[t, m])}
            for tn, ts in multi:
                combined[name_of(name, "AP", tn, m)] = nanmean([ap[t, m] for t in ts])
                if has_classes:
                    combined[name_of(name, "mAP", tn, m)] = nanmean([nanmean(cap[t, m]) for t in ts])
    for group, names in ((confusions, confusion_names if confusion_names is not None else class_names),
                         (overlap_confusions, class_names)):
        for name, m in group.items():
            iou, avg = confusion_iou(m)
            combined[f"{name}_avg_iou"] = avg
            single_class[f"{name}_iou"] = {f"{names[i]}": v for i, v in enumerate(iou)}
    for name, (conf, labels) in binaries.items():
        _, iou, avg, _, mean_avg = binary_collection(conf, labels, class_indices)
        combined[f"{name}_mean_avg_iou"] = mean_avg
        combined[f"{name}_average_iou"] = avg
        single_class[f"{name}_iou"] = {f"{class_names[i]}": v for i, v in enumerate(iou)}
    return combined, single_class, n_points


def same_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))


def max_diff(a, b):
    """Largest |a - b| over the entries that are numbers in both (NaN places are compared with same_nan)."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    ok = ~(np.isnan(a) | np.isnan(b))
    return float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0


# ---- the fixtures (tests/golden/eval_*.npz, written by tests/golden/make_eval_golden.py) -------------------------------------
OVERLAP_NAMES = ("bbox", "gtbbox", "mask", "gtmask", "gtlabelmask")


def load_case(path):
    """-> (z, samples): per sample the bool masks, int64 classes, fp32 scores and boxes the reference was given."""
    z = np.load(path)
    samples, o = [], dict(p=0, g=0, n=0)
    for s, (n, g, p) in enumerate(zip(z["n_points"], z["n_gt"], z["n_pred"])):
        n, g, p = int(n), int(g), int(p)
        d = dict(n=n, gt=unpack_rows(z[f"gt_bits_{s}"], g, n), pred=unpack_rows(z[f"pred_bits_{s}"], p, n),
                 gtbox_mask=unpack_rows(z[f"gtbox_mask_bits_{s}"], g, n), gtlabel_mask=unpack_rows(z[f"gtlabel_mask_bits_{s}"], g, n),
                 labels=z["labels"][o["g"]:o["g"] + g].astype(np.int64), gt_bbox_class=z["gt_bbox_class"][o["g"]:o["g"] + g].astype(np.int64),
                 gtb=z["gtb"][o["g"]:o["g"] + g], pcls=z["pcls"][o["p"]:o["p"] + p].astype(np.int64),
                 score=z["score"][o["p"]:o["p"] + p], pb=z["pb"][o["p"]:o["p"] + p],
                 seg_gt=z["seg_gt"][o["n"]:o["n"] + n].astype(np.int64), seg_pred=z["seg_pred"][o["n"]:o["n"] + n].astype(np.int64))
        samples.append(d)
        o["p"] += p
        o["g"] += g
        o["n"] += n
    return z, samples


def thresholds_of(z):
    return [float(t) for t in z["single_thresholds"]] + [(str(z["multi_name"]), tuple(float(t) for t in z["multi_thresholds"]))]


def case_records(z, samples):
    """The five overlap accumulators of training.py's AccumulatorCollection as lists of records (unfiltered + keep flag)."""
    thr = float(z["score_threshold"])
    recs = {n: [] for n in OVERLAP_NAMES}
    for s in samples:
        ones = np.ones(len(s["gt"]), np.float32)
        keep = s["score"] >= np.float32(thr)
        recs["bbox"].append(dict(score=s["score"], iou=box_iou(s["pb"], s["gtb"]), keep=keep, pred_class=s["pcls"], gt_class=s["labels"]))
        recs["mask"].append(dict(score=s["score"], iou=mask_iou(s["pred"], s["gt"]), keep=keep, pred_class=s["pcls"], gt_class=s["labels"]))
        recs["gtbbox"].append(dict(score=ones, iou=box_iou(s["gtb"], s["gtb"]), keep=ones >= thr, pred_class=s["gt_bbox_class"], gt_class=s["labels"]))
        recs["gtmask"].append(dict(score=ones, iou=mask_iou(s["gtbox_mask"], s["gt"]), keep=ones >= thr, pred_class=s["gt_bbox_class"], gt_class=s["labels"]))
        recs["gtlabelmask"].append(dict(score=ones, iou=mask_iou(s["gtlabel_mask"], s["gt"]), keep=ones >= thr, pred_class=s["labels"], gt_class=s["labels"]))
    return recs


def case_flags(recs, thresholds, classes):
    """-> ([thresholds, kept predictions], [thresholds, class-major flags], num_gt per class): the fixtures' tp_ / tpc_ layout."""
    tp = np.stack([np.concatenate([problem(r, t)[1] for r in recs]) for t in thresholds])
    tpc = np.stack([np.concatenate([problem(r, t, c)[1] for c in classes for r in recs]) for t in thresholds])
    return tp, tpc, np.array([sum(problem(r, thresholds[0], c)[2] for r in recs) for c in classes], np.int64)


def case_metrics(z, samples, recs=None):
    """-> (combined, single_class, n_curve_points, confusions) of a fixture case, restated."""
    recs = case_records(z, samples) if recs is None else recs
    k, seg = int(z["k"]), int(z["seg"])
    conf = dict(segment=confusion(np.concatenate([s["seg_pred"] for s in samples]), np.concatenate([s["seg_gt"] for s in samples]), seg),
                gtbbox=confusion(np.concatenate([s["gt_bbox_class"] for s in samples]), np.concatenate([s["labels"] for s in samples]), k),
                gtlabelmask=np.concatenate([pair_confusion(s["gtlabel_mask"], s["gt"]) for s in samples]))
    labels = np.concatenate([s["labels"] for s in samples])
    combined, single_class, n_points = metrics(recs, {"segment": conf["segment"]}, {"gtbbox": conf["gtbbox"]},
                                               {"gtlabelmask": (conf["gtlabelmask"], labels)}, thresholds_of(z), list(range(k)),
                                               [str(n) for n in z["class_names"]], (None, 11), [str(n) for n in z["seg_names"]])
    combined = {key: v for key, v in combined.items() if "gtbbox_AP" not in key}
    return combined, single_class, n_points, conf


def expected_metrics(z):
    """The reference's dictionaries as the fixture stores them."""
    combined = dict(zip([str(k) for k in z["combined_keys"]], z["combined_values"]))
    single_class = {}
    for i, key in enumerate(str(k) for k in z["single_class_keys"]):
        names = z["seg_names"] if key == "segment_iou" else z["class_names"]
        single_class[key] = dict(zip([str(n) for n in names], z[f"single_class_{i}"]))
    return combined, single_class


def compare_metrics(got, want, bound, label=""):
    """Same keys, NaN where `want` has NaN, numbers within `bound`; -> the worst difference."""
    (gc, gs), (wc, ws) = got, want
    assert set(gc) == set(wc), (sorted(set(gc) ^ set(wc)))
    assert set(gs) == set(ws), (sorted(set(gs) ^ set(ws)))
    worst = 0.0
    for key in wc:
        assert same_nan(gc[key], wc[key]), (label, key, gc[key], wc[key])
        worst = max(worst, max_diff(gc[key], wc[key]))
    for key in ws:
        assert [str(n) for n in gs[key]] == [str(n) for n in ws[key]], (label, key)
        a, b = np.array([float(v) for v in gs[key].values()]), np.array([float(v) for v in ws[key].values()])
        assert same_nan(a, b), (label, key, a, b)
        worst = max(worst, max_diff(a, b))
    assert worst <= bound, (label, worst, bound)
    return worst
