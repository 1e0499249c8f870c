"""Generates the evaluation fixtures by RUNNING the reference's own code on the CPU (build container only, needs
/root/reference; `import sparseconvnet` is satisfied by this repository's package):

    python tests/golden/make_eval_golden.py

  eval_<case>.npz   seeded inputs (masks as np.packbits of the thresholded bool masks -- the dense fp32 prediction the reference
                    is given is 0.75 where the bit is set and 0.25 elsewhere --, scores, classes, boxes, segmentation labels)
                    and the outputs of ndsis/training/evaluation.py: the IoU matrices of MaskOverlapCalculator /
                    BboxOverlapCalculator, calc_tp_indicator's flags per threshold (classless and class-wise), the
                    PrecisionRecallCurve of every overlap metric, every entry of EvaluationHelper's combined_metrics and
                    single_class_metrics (class names passed explicitly), the segmentation / label confusion matrices and the
                    binary mask confusion tensors.
Cases: basic, empty (a sample without predictions, one without ground truth, a class with ground truth and no prediction, a
class with neither), nan (an empty predicted mask against an empty ground-truth mask: IoU 0 / 0, at the top score), ties_iou
(two identical ground truths: equal IoU to one prediction), boxes (more boxes, from make_mask_loss_golden's generators).

TIE RULE.  The reference sorts a data set's scores with an unstable `score.sort(descending=True)`; the pseudo-score metrics
(gtbbox, gtmask, gtlabelmask: every score is 1 in training.py) would depend on that accident.  The package's rule is "equal
scores keep accumulation order".  So the reference is GIVEN pseudo-scores that already say so: 1 - i * 2^-20 for the i-th
ground truth of the data set, distinct and descending in accumulation order.  Its own code then runs unchanged, and the
fixtures store the pseudo-score curves' scores as the ones the package is given.
The `nan` case also stores two hand-written overlap matrices (`rule_iou_*`) with the reference's calc_tp_indicator flags:
a NaN can only stand in a row that would otherwise match when the matrix is given (an empty mask overlaps nothing else).
The `ties_iou` case: prediction 0 covers ground truths 0 and 1 (equal sizes, IoU 0.5 with both), prediction 1 is ground truth
0 exactly -- under "first index wins" prediction 1 is a false positive, under "last index wins" it would be a true one.
Only inputs and outputs are stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)

K, SEG = 18, 20
SCORE_THR, MASK_THR = 0.65, 0.5
SINGLE = [0.25, 0.5]
MULTI = ("[0.5:0.95:0.05]", (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95))
CLASS_NAMES = [f"c{i}" for i in range(K)]
SEG_NAMES = [f"s{i}" for i in range(SEG)]
OVERLAP_NAMES = ("bbox", "gtbbox", "mask", "gtmask", "gtlabelmask")


def noisy_copy(rng, m, drop, add):
    out = m & (rng.uniform(size=m.shape) > drop)
    return out | (rng.uniform(size=m.shape) < add * max(m.mean(), 1e-3))


def make_sample(rng, n, g, p, grid, special=None):
    from make_mask_loss_golden import boxes_near, random_boxes
    inst = rng.integers(-1, max(g, 1), size=n) if g else np.full(n, -1)
    if special == "nan" and g:
        inst[inst == 0] = -1                                   # ground truth 0: an empty mask
    gt = inst[None, :] == np.arange(g)[:, None]
    labels = rng.integers(0, K - 1, size=g).astype(np.int64)   # (class 17 is placed by hand)
    if special == "ties_iou":                                  # ground truths 0 and 1: disjoint, equally large, one class
        i0, i1 = np.nonzero(gt[0])[0], np.nonzero(gt[1])[0]
        m = min(len(i0), len(i1))
        gt[0, i0[m:]] = False
        gt[1, i1[m:]] = False
        labels[1] = labels[0]
    if special == "empty" and g:
        labels[0] = K - 1                                      # a class with ground truth that nothing predicts
    pred = np.zeros((p, n), bool)
    pcls = np.zeros(p, np.int64)
    good = rng.permutation(p) < int(0.6 * p) if g else np.zeros(p, bool)
    for i in range(p):
        if good[i]:
            src = int(rng.integers(g))
            pred[i] = noisy_copy(rng, gt[src], rng.uniform(0.02, 0.7), rng.uniform(0, 0.3))
            pcls[i] = labels[src] if rng.uniform() < 0.8 else rng.integers(K - 1)
        else:
            pred[i] = rng.uniform(size=n) < rng.uniform(0.01, 0.1)
            pcls[i] = rng.integers(K - 1)
    if special == "ties_iou":
        pred[0], pcls[0] = gt[0] | gt[1], labels[0]            # IoU exactly 0.5 with both
        pred[1], pcls[1] = gt[0].copy(), labels[0]             # IoU 1 with ground truth 0, 0 with ground truth 1
    if special == "nan" and p:
        pred[0] = False                                        # the top score: an empty mask, IoU NaN with ground truth 0
    score = np.sort(rng.uniform(0.55, 1.0, p).astype(np.float32))[::-1].copy()
    assert len(np.unique(score)) == p
    gtb = random_boxes(rng, g, grid, 3.0, 0.7 * min(grid))
    n_near = int(0.6 * p) if g else 0
    pb = np.concatenate([boxes_near(rng, gtb, n_near, 0.15), random_boxes(rng, p - n_near, grid, 2.0, 10.0)])
    pb = pb[rng.permutation(p)] if p else pb
    gt_bbox_class = np.where(rng.uniform(size=g) < 0.7, labels, rng.integers(0, K, size=g)).astype(np.int64)
    gtbox_mask = np.stack([noisy_copy(rng, gt[i], rng.uniform(0.05, 0.6), 0.2) for i in range(g)]) if g else gt.copy()
    gtlabel_mask = np.stack([noisy_copy(rng, gt[i], rng.uniform(0.05, 0.4), 0.1) for i in range(g)]) if g else gt.copy()
    if special == "nan" and g:
        gtlabel_mask[0] = False                                # a pair with an empty union
    seg_gt = rng.integers(0, SEG, size=n).astype(np.int64)
    seg_pred = np.where(rng.uniform(size=n) < 0.6, seg_gt, rng.integers(0, SEG, size=n)).astype(np.int64)
    seg_gt[rng.uniform(size=n) < 0.1] = -100
    return dict(gt=gt, labels=labels, pred=pred, pcls=pcls, score=score, gtb=gtb.reshape(-1, 2, 3), pb=pb.reshape(-1, 2, 3),
                gt_bbox_class=gt_bbox_class, gtbox_mask=gtbox_mask, gtlabel_mask=gtlabel_mask, seg_gt=seg_gt, seg_pred=seg_pred)


def dense(bits):
    return torch.from_numpy(np.where(bits, np.float32(0.75), np.float32(0.25)))


def main():
    sys.path.insert(0, "/root/reference")
    import sparse_rcnn_amd
    sys.modules["sparseconvnet"] = sparse_rcnn_amd
    from ndsis.training import evaluation as RE

    def case(name, seed, grid, n_points, n_gt, n_pred, special=None, check=False):
        rng = np.random.default_rng(seed)
        S = [make_sample(rng, n, g, p, grid, special if s == 0 else None) for s, (n, g, p) in enumerate(zip(n_points, n_gt, n_pred))]
        T = torch.from_numpy
        bbox_calc = RE.BboxOverlapCalculator(score_threshold=SCORE_THR)
        mask_calc = RE.MaskOverlapCalculator(MASK_THR, score_threshold=SCORE_THR)
        acc = {n: RE.OverlapAccumulator(bbox_calc if "bbox" in n else mask_calc) for n in OVERLAP_NAMES}
        seg_acc = RE.ConfusionAccumulator(RE.ConfusionCalculator(SEG))
        label_acc = RE.ConfusionAccumulator(RE.ConfusionCalculator(K))
        bin_acc = RE.BinaryConfusionAccumulator(RE.BinaryMaskConfusionCalculator(MASK_THR))
        first = np.concatenate([[0], np.cumsum(n_gt)])
        pseudo = [torch.from_numpy((1.0 - (first[i] + np.arange(len(s["gt"]))) * 2.0 ** -20).astype(np.float32))
                  for i, s in enumerate(S)]                      # (see TIE RULE above; all above the score threshold)
        assert len(np.unique(np.concatenate([s["score"] for s in S]))) == sum(n_pred)
        gtl = [T(s["labels"]) for s in S]
        gtm = [T(s["gt"]) for s in S]
        gtbox = [T(s["gtb"]) for s in S]
        acc["bbox"].add_batch([T(s["score"]) for s in S], [T(s["pb"]) for s in S], gtbox, [T(s["pcls"]) for s in S], gtl)
        acc["gtbbox"].add_batch(pseudo, gtbox, gtbox, [T(s["gt_bbox_class"]) for s in S], gtl)
        label_acc.add_list_batch([T(s["gt_bbox_class"]) for s in S], gtl)
        acc["mask"].add_batch([T(s["score"]) for s in S], [dense(s["pred"]) for s in S], gtm, [T(s["pcls"]) for s in S], gtl)
        acc["gtmask"].add_batch(pseudo, [dense(s["gtbox_mask"]) for s in S], gtm, [T(s["gt_bbox_class"]) for s in S], gtl)
        acc["gtlabelmask"].add_batch(pseudo, [dense(s["gtlabel_mask"]) for s in S], gtm, gtl, gtl)
        bin_acc.add_batch([dense(s["gtlabel_mask"]) for s in S], gtm, gtbox, gtl)
        seg_acc.add_batch(torch.cat([T(s["seg_pred"]) for s in S]), torch.cat([T(s["seg_gt"]) for s in S]))
        helper = RE.EvaluationHelper([*SINGLE, MULTI], list(range(K)), CLASS_NAMES, [None, 11], SEG_NAMES)
        combined, single_class, _, conf, oconf, binary = helper(acc, {"segment": seg_acc}, {"gtbbox": label_acc},
                                                                {"gtlabelmask": bin_acc})
        combined = {k: v for k, v in combined.items() if "gtbbox_AP" not in k}      # training.py:174-177
        out = dict(k=np.array(K), seg=np.array(SEG), score_threshold=np.array(SCORE_THR), mask_threshold=np.array(MASK_THR),
                   single_thresholds=np.array(SINGLE), multi_name=np.array(MULTI[0]), multi_thresholds=np.array(MULTI[1]),
                   class_names=np.array(CLASS_NAMES), seg_names=np.array(SEG_NAMES),
                   n_points=np.array(n_points, np.int64), n_gt=np.array(n_gt, np.int64), n_pred=np.array(n_pred, np.int64))
        for key in ("labels", "pcls", "score", "gtb", "pb", "gt_bbox_class", "seg_gt", "seg_pred"):
            out[key] = np.concatenate([s[key] for s in S])
            if out[key].dtype == np.int64:
                out[key] = out[key].astype(np.int8)             # (classes and -100 fit; read back as int64)
        full_bbox, full_mask = RE.BboxOverlapCalculator(), RE.MaskOverlapCalculator(MASK_THR)
        for i, s in enumerate(S):
            for key in ("gt", "pred", "gtbox_mask", "gtlabel_mask"):
                out[f"{key}_bits_{i}"] = np.packbits(s[key], axis=1)
            out[f"mask_iou_{i}"] = full_mask(T(s["score"]), dense(s["pred"]), T(s["gt"]), T(s["pcls"]))[1].numpy()
            out[f"box_iou_{i}"] = full_bbox(T(s["score"]), T(s["pb"]), T(s["gtb"]), T(s["pcls"]))[1].numpy()
            out[f"gtmask_iou_{i}"] = full_mask(pseudo[i], dense(s["gtbox_mask"]), T(s["gt"]), None)[1].numpy()
        thresholds = helper.overlap_thresholds
        out["thresholds"] = np.array(thresholds)
        tpi = RE.PrecisionRecallCurve.calc_tp_indicator
        for n in OVERLAP_NAMES:
            a = acc[n]
            cw = a.get_classwise_accumulator(list(range(K)))
            # [thresholds, kept predictions (sample-major)] and [thresholds, (class-major, sample, kept prediction of the class)]
            out[f"tp_{n}"] = np.stack([np.concatenate([tpi(i, t).numpy() for i in a.iou_list]) for t in thresholds])
            out[f"tpc_{n}"] = np.stack([np.concatenate([tpi(i, t).numpy() for iou_list in cw.sorted_iou_list_list
                                                        for i in iou_list]) for t in thresholds])
            out[f"class_num_gt_{n}"] = np.array([c.num_gt for c in cw.get_pr_collection(thresholds[0])], np.int64)
            for t in SINGLE:
                c = a.get_pr_curve(t)
                out[f"curve_{n}_{t}_score"], out[f"curve_{n}_{t}_tp"] = c.score.numpy(), c.tp_indicator.numpy()
                if n.startswith("gt"):
                    out[f"curve_{n}_{t}_score"] = np.ones_like(out[f"curve_{n}_{t}_score"])
                out[f"curve_{n}_{t}_precision"], out[f"curve_{n}_{t}_recall"] = c.precision.numpy(), c.recall.numpy()
                out[f"curve_{n}_{t}_interpolated"], out[f"curve_{n}_{t}_num_gt"] = c.precision_interpolated.numpy(), np.array(c.num_gt)
            out[f"kept_{n}"] = np.array([len(s) for s in a.score_list], np.int64)
        out["combined_keys"] = np.array(list(combined))
        out["combined_values"] = np.array([float(combined[k]) for k in combined], np.float64)
        out["single_class_keys"] = np.array(list(single_class))
        for i, k in enumerate(single_class):
            d = single_class[k]
            names = SEG_NAMES if k == "segment_iou" else CLASS_NAMES
            assert list(d) == names, (k, list(d))
            out[f"single_class_{i}"] = np.array([float(d[n]) for n in names], np.float64)
        out["segment_confusion"] = conf["segment"].confusion_matrix
        out["gtbbox_confusion"] = oconf["gtbbox"].confusion_matrix
        out["gtlabelmask_confusion"] = torch.stack(bin_acc.confusion_matrix_list).numpy() if bin_acc.confusion_matrix_list \
            else np.zeros((0, 2, 2), np.int64)
        out["gtlabelmask_classwise"] = binary["gtlabelmask"].classwise_confusion_matrices
        out["gtlabelmask_classwise_mean_iou"] = binary["gtlabelmask"].classwise_mean_iou

        # a fixture that matches nothing tests nothing
        i05 = thresholds.index(0.5)
        tp = out["tp_mask"][i05]
        kept, total = int(out["kept_mask"].sum()), int(sum(n_pred))
        cap = out[f"single_class_{list(single_class).index('mask_class_AP_0.5')}"]
        facts = dict(tp=int(tp.sum()), fp=int((~tp).sum()), kept=kept, total=total, ap_zero=int((cap == 0).sum()),
                     ap_nan=int(np.isnan(cap).sum()), ap_pos=int((cap > 0).sum()),
                     nan_iou=int(sum(np.isnan(out[f"mask_iou_{i}"]).sum() for i in range(len(S)))))
        if check:
            assert facts["tp"] >= 1 and facts["fp"] >= 1, facts
            assert kept < total and 2 * kept >= total, facts
            assert facts["ap_zero"] >= 1 and facts["ap_nan"] >= 1, facts
            tb = out["tp_bbox"][i05]
            assert tb.any() and not tb.all(), "boxes: no true or no false positive"
        if special == "nan":
            assert np.isnan(out["mask_iou_0"][0, 0]) and facts["nan_iou"] >= 1, facts
            r2 = np.random.default_rng(seed + 100)
            given = [np.array([[np.nan, .9], [.8, .7]], np.float32), np.round(r2.uniform(0, 1, (14, 6)), 1).astype(np.float32)]
            given[1][r2.uniform(size=given[1].shape) < 0.08] = np.nan
            given[1][0, :2] = (np.nan, 0.9)                      # the NaN row would otherwise have matched
            for i, m in enumerate(given):
                out[f"rule_iou_{i}"] = m
                out[f"rule_tp_{i}"] = np.stack([RE.PrecisionRecallCurve.calc_tp_indicator(T(m), t).numpy() for t in thresholds])
            assert out["rule_tp_0"][thresholds.index(0.5)].tolist() == [False, True] and not out["rule_tp_1"][:, 0].any()
            assert out["rule_tp_1"].any()
        if special == "ties_iou":
            m = out["mask_iou_0"]
            assert m[0, 0] == m[0, 1] == 0.5 and m[1, 0] == 1 and m[1, 1] == 0, m[:2, :2]
            assert tp[0] and not tp[1], tp[:2]                   # first index wins; last index would make both true
        path = os.path.join(HERE, f"eval_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {facts} mask_AP_0.5 {combined['mask_AP_0.5']:.4f} mask_mAP_0.5 {combined['mask_mAP_0.5']:.4f} "
              f"bbox_AP_0.5 {combined['bbox_AP_0.5']:.4f} {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 100_000

    case("basic", 0, (40, 32, 24), [2000, 1600, 1400], [7, 5, 9], [30, 28, 32], check=True)
    case("empty", 1, (32, 32, 16), [2000, 1500, 1800], [6, 5, 0], [24, 0, 20], special="empty")
    case("nan", 2, (32, 24, 16), [2200, 1700], [6, 5], [26, 22], special="nan")
    case("ties_iou", 3, (32, 24, 16), [2400, 1600], [6, 7], [25, 27], special="ties_iou")
    case("boxes", 4, (48, 40, 32), [600, 500], [9, 8], [60, 50], check=True)


if __name__ == "__main__":
    main()
