"""GPU: the evaluation on the device (csrc/scn_eval.hip behind sparse_rcnn_amd.evaluation, SceneStep.evaluate) against the
reference's own outputs (tests/golden/eval_*.npz) and, at size, against the numpy restatement that the CPU suite pins to those
fixtures (tests/eval_restate.py).

Bounds: IoU matrices, true-positive flags, sorted order, num_gt, confusion tensors, precision and recall are compared for
EQUALITY (integers, or one correctly rounded fp32 division of two exact integers).  AP / mAP / mean IoU: n * 2^-24 absolute for
a curve of n points -- only the order of the final fp32 sum of terms that total <= 1 can differ."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eval_restate as ER                                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CASES = sorted(glob.glob(os.path.join(HERE, "golden", "eval_*.npz")))


def _id(p):
    return os.path.basename(p)[5:-4]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dense(bits):
    return T(np.where(bits, np.float32(0.75), np.float32(0.25)))


def same(t, want):
    """torch.equal with NaNs at the same places."""
    want = T(want)
    if t.shape != want.shape or t.dtype != want.dtype:
        return False
    if t.is_floating_point():
        return bool(torch.equal(torch.isnan(t), torch.isnan(want)) and torch.equal(torch.nan_to_num(t), torch.nan_to_num(want)))
    return bool(torch.equal(t, want))


def packed(masks, E):
    """list of bool [rows, n] -> list of PackedSample in one buffer (the restatement's word layout, uploaded)."""
    words = [ER.words_of(m) for m in masks]
    offs = np.concatenate([[0], np.cumsum([w.size for w in words])])
    base = T(np.concatenate([w.reshape(-1) for w in words] + [np.zeros(1, np.uint32)]).view(np.int32))
    return [E.PackedSample(base, offs[i], m.shape[0], m.shape[1]) for i, m in enumerate(masks)]


def build_accumulators(z, samples, E, packed_inputs):
    """training.py's AccumulatorCollection.add_batch on this package's classes."""
    st, mt = float(z["score_threshold"]), float(z["mask_threshold"])
    bbox_calc, mask_calc = E.BboxOverlapCalculator(score_threshold=st), E.MaskOverlapCalculator(mt, score_threshold=st)
    acc = {n: E.OverlapAccumulator(bbox_calc if "bbox" in n else mask_calc) for n in ER.OVERLAP_NAMES}
    seg_acc, label_acc = E.ConfusionAccumulator(E.ConfusionCalculator(int(z["seg"]))), E.ConfusionAccumulator(E.ConfusionCalculator(int(z["k"])))
    bin_acc = E.BinaryConfusionAccumulator(E.BinaryMaskConfusionCalculator(mt))
    S = samples
    pseudo = [torch.ones(len(s["gt"]), device=DEV) for s in S]
    gtl, gtbox = [T(s["labels"]) for s in S], [T(s["gtb"]) for s in S]
    if packed_inputs:
        gtm = E.pack_gt_masks([T(s["gt"]) for s in S])
        pm = {k: packed([s[k] for s in S], E) for k in ("pred", "gtbox_mask", "gtlabel_mask")}
    else:
        gtm = [T(s["gt"]) for s in S]
        pm = {k: [dense(s[k]) for s in S] for k in ("pred", "gtbox_mask", "gtlabel_mask")}
    acc["bbox"].add_batch([T(s["score"]) for s in S], [T(s["pb"]) for s in S], gtbox, [T(s["pcls"]) for s in S], gtl)
    acc["gtbbox"].add_batch(pseudo, gtbox, gtbox, [T(s["gt_bbox_class"]) for s in S], gtl)
    label_acc.add_list_batch([T(s["gt_bbox_class"]) for s in S], gtl)
    acc["mask"].add_batch([T(s["score"]) for s in S], pm["pred"], gtm, [T(s["pcls"]) for s in S], gtl)
    acc["gtmask"].add_batch(pseudo, pm["gtbox_mask"], gtm, [T(s["gt_bbox_class"]) for s in S], gtl)
    acc["gtlabelmask"].add_batch(pseudo, pm["gtlabel_mask"], gtm, gtl, gtl)
    bin_acc.add_batch(pm["gtlabel_mask"], gtm, gtbox, gtl)
    seg_acc.add_batch(torch.cat([T(s["seg_pred"]) for s in S]), torch.cat([T(s["seg_gt"]) for s in S]))
    return acc, seg_acc, label_acc, bin_acc


# ---- 1. kernels and public classes against the fixtures --------------------------------------------------------------------
@pytest.mark.parametrize("path", CASES, ids=_id)
def test_overlap_matrices_equal_the_reference(path):
    from sparse_rcnn_amd import evaluation as E
    z, S = ER.load_case(path)
    mt = float(z["mask_threshold"])
    boxes = E.bbox_iou([T(s["pb"]) for s in S], [T(s["gtb"]) for s in S])
    r_dense = E.mask_iou(E.pack_threshold([dense(s["pred"]) for s in S], mt), E.pack_gt_masks([T(s["gt"]) for s in S]))
    r_packed = E.mask_iou(packed([s["pred"] for s in S], E), packed([s["gt"] for s in S], E))
    for s, d in enumerate(S):
        assert same(boxes[s], z[f"box_iou_{s}"]), s
        for r in (r_dense, r_packed):
            got = r.sample(s)
            assert same(got["iou"], z[f"mask_iou_{s}"]), s
            inter, pc, gc = ER.mask_counts(d["pred"], d["gt"])
            assert same(got["inter"], inter.astype(np.int32)) and same(got["pred_count"], pc.astype(np.int32))
            assert same(got["gt_count"], gc.astype(np.int32))
        # the calculators, called as the reference calls them: the compacted tensors
        sc, iou, pc = E.MaskOverlapCalculator(mt, score_threshold=float(z["score_threshold"]))(
            T(d["score"]), dense(d["pred"]), T(d["gt"]), T(d["pcls"]))
        keep = d["score"] >= np.float32(z["score_threshold"])
        assert same(iou, z[f"mask_iou_{s}"][keep]) and same(sc, d["score"][keep]) and same(pc, d["pcls"][keep])
        sc, iou, _ = E.MaskOverlapCalculator(mt)(torch.ones(len(d["gt"]), device=DEV), dense(d["gtbox_mask"]), T(d["gt"]), None)
        assert same(iou, z[f"gtmask_iou_{s}"])
        sc, iou, pc = E.BboxOverlapCalculator(sort=True)(T(d["score"][::-1].copy()), T(d["pb"][::-1].copy()), T(d["gtb"]),
                                                          T(d["pcls"][::-1].copy()))
        assert same(iou, z[f"box_iou_{s}"]) and same(sc, d["score"]) and same(pc, d["pcls"])
        fm = E.MaskOverlapCalculator(mt, filter_masks=True)(T(d["score"]), dense(d["pred"]), T(d["gt"]), T(d["pcls"]))
        assert same(fm[1], z[f"mask_iou_{s}"][d["pred"].any(1)])


@pytest.mark.parametrize("packed_inputs", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("path", CASES, ids=_id)
def test_flags_curves_and_metrics_equal_the_reference(path, packed_inputs):
    from sparse_rcnn_amd import evaluation as E
    z, S = ER.load_case(path)
    k = int(z["k"])
    acc, seg_acc, label_acc, bin_acc = build_accumulators(z, S, E, packed_inputs)
    thresholds = [float(t) for t in z["thresholds"]]
    for n in ER.OVERLAP_NAMES:
        recs = acc[n].records
        flags, num_gt = E.match([r["iou"] for r in recs], thresholds, [r["keep"] for r in recs], [r["pred_class"] for r in recs],
                                [r["gt_class"] for r in recs], range(k))
        flags2, num_gt2 = E.match([r["iou"] for r in recs], thresholds, [r["keep"] for r in recs],
                                  [r["pred_class"] for r in recs], [r["gt_class"] for r in recs], range(k))
        assert torch.equal(flags, flags2) and torch.equal(num_gt, num_gt2)
        f, ng = flags.cpu().numpy(), num_gt.cpu().numpy()
        assert np.array_equal(np.stack([f[0, t][f[0, t] >= 0] > 0 for t in range(len(thresholds))]), z[f"tp_{n}"]), n
        tpc = np.stack([np.concatenate([f[1 + c, t][f[1 + c, t] >= 0] > 0 for c in range(k)]) for t in range(len(thresholds))])
        assert np.array_equal(tpc, z[f"tpc_{n}"]), n
        assert np.array_equal(ng[1:, 0].sum(-1), z[f"class_num_gt_{n}"]), n
        assert np.array_equal(acc[n].get_counts()[:, 0], z[f"kept_{n}"]), n
        for t in (float(t) for t in z["single_thresholds"]):
            c = acc[n].get_pr_curve(t)
            assert c.num_gt == int(z[f"curve_{n}_{t}_num_gt"])
            assert np.array_equal(c.score.cpu().numpy(), z[f"curve_{n}_{t}_score"]), (n, t)
            assert np.array_equal(c.tp_indicator.cpu().numpy(), z[f"curve_{n}_{t}_tp"]), (n, t)
            for got, key in ((c.precision, "precision"), (c.recall, "recall"), (c.precision_interpolated, "interpolated")):
                assert np.array_equal(got.cpu().numpy(), z[f"curve_{n}_{t}_{key}"], equal_nan=True), (n, t, key)
    helper = E.EvaluationHelper(ER.thresholds_of(z), list(range(k)), [str(x) for x in z["class_names"]], [None, 11],
                                [str(x) for x in z["seg_names"]])
    combined, single_class, _, conf, oconf, binary = helper(acc, {"segment": seg_acc}, {"gtbbox": label_acc},
                                                            {"gtlabelmask": bin_acc})
    combined = {key: v for key, v in combined.items() if "gtbbox_AP" not in key}
    assert np.array_equal(conf["segment"].confusion_matrix, z["segment_confusion"])
    assert np.array_equal(oconf["gtbbox"].confusion_matrix, z["gtbbox_confusion"])
    got_bin = torch.cat(bin_acc.confusion_matrix_list).cpu().numpy() if bin_acc.confusion_matrix_list else np.zeros((0, 2, 2))
    assert np.array_equal(got_bin, z["gtlabelmask_confusion"])
    assert np.array_equal(binary["gtlabelmask"].classwise_confusion_matrices, z["gtlabelmask_classwise"])
    n_curve = max(max(int(a.get_counts()[:, 0].sum()) for a in acc.values()), int(z["seg"]))
    worst = ER.compare_metrics((combined, single_class), ER.expected_metrics(z), ER.ap_bound(n_curve), _id(path))
    print(f"{_id(path)} ({'packed' if packed_inputs else 'dense'}): worst metric difference {worst:.3e} "
          f"(bound {ER.ap_bound(n_curve):.3e})")


def test_matching_rules_nan_tie_and_order():
    from sparse_rcnn_amd.evaluation import PrecisionRecallCurve, match
    z = np.load(os.path.join(HERE, "golden", "eval_nan.npz"))      # hand-written matrices, flags by the reference's own loop
    for i in range(2):
        flags, _ = match([T(z[f"rule_iou_{i}"])], [float(t) for t in z["thresholds"]])
        assert np.array_equal(flags[0].cpu().numpy() > 0, z[f"rule_tp_{i}"]), i
    tp = PrecisionRecallCurve.calc_tp_indicator(T(np.array([[np.nan, .9], [.8, .7]], np.float32)), 0.5)
    assert tp.tolist() == [False, True]
    assert PrecisionRecallCurve.calc_tp_indicator(T(np.array([[.6, .6], [.6, .1]], np.float32)), 0.5).tolist() == [True, False]
    rng = np.random.default_rng(5)
    for p, g in ((40, 70), (3, 200), (130, 65)):                 # more ground truths than lanes
        m = np.round(rng.uniform(0, 1, (p, g)), 1).astype(np.float32)        # many exact ties
        m[rng.uniform(size=m.shape) < 0.01] = np.nan
        for t in (0.3, 0.7):
            flags, num_gt = match([T(m)], [t])
            assert np.array_equal(flags[0, 0].cpu().numpy() > 0, ER.match(m, t)) and int(num_gt[0, 0, 0]) == g


# ---- 2. the packed predictions equal the dense ones, bit for bit -----------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.5, 0.3])
def test_mask_bits_equal_mask_predict_thresholded(threshold):
    from sparse_rcnn_amd import evaluation as E, roi
    rng = np.random.default_rng(11)
    splits, counts, k = [1237, 901], [5, 4], 18
    n, bb = sum(splits), sum(counts)
    inside = np.zeros((bb, n), bool)
    starts, b = np.concatenate([[0], np.cumsum(splits)]), 0
    for s, c in enumerate(counts):
        for _ in range(c):
            inside[b, starts[s]:starts[s + 1]] = rng.uniform(size=splits[s]) < rng.uniform(0.05, 0.6)
            b += 1
    inside[2] = False                                            # an empty box
    sel = roi.selection_from_matrix(torch.from_numpy(inside))
    logits = T((rng.standard_normal((int(inside.sum()), k)) * 2).astype(np.float32))
    cls = rng.integers(0, k, size=bb).astype(np.int64)
    cls[1], cls[6] = -1, k - 1                                   # invalid: negative, and beyond num_valid below
    for num_valid in (0, k - 1):
        want = roi.mask_predict(logits, sel, counts, splits, torch.from_numpy(cls), num_valid)
        got = E.mask_bits(logits, sel, counts, splits, torch.from_numpy(cls), num_valid, threshold)
        again = E.mask_bits(logits, sel, counts, splits, torch.from_numpy(cls), num_valid, threshold)
        repacked = E.pack_threshold(want, threshold)
        n_words = got.word_offsets[-1]
        assert torch.equal(got.words[:n_words], again.words[:n_words])
        assert torch.equal(got.words[:n_words], repacked.words[:n_words]) and got.word_offsets == repacked.word_offsets
        for s, ps in enumerate(E.split_packed(got)):
            assert torch.equal(ps.unpack(), want[s] > threshold)
            assert (want[s] > threshold).any()
        w = E.split_packed(got)[0].words                         # the bits beyond N in a row's last word are zero
        assert int((w[:, -1].to(torch.int64) & 0xFFFFFFFF).max()) < (1 << (splits[0] % 32))
        assert not E.split_packed(got)[0].unpack()[1].any() and not E.split_packed(got)[0].unpack()[2].any()


# ---- 3. at size against the restatement --------------------------------------------------------------------------------------
def _at_size_masks(rng, p, g, n):
    gt = rng.uniform(size=(g, n)) < rng.uniform(0.001, 0.3, (g, 1))
    pred = rng.uniform(size=(p, n)) < rng.uniform(0.001, 0.3, (p, 1))
    for i in range(0, p, 2):                                     # every other prediction: a noisy copy of a ground truth
        pred[i] = gt[i % g] & (rng.uniform(size=n) > rng.uniform(0.05, 0.8))
    return pred, gt


@pytest.mark.parametrize("shape", [(1, 64, 64, 172_500), (1, 256, 64, 172_500), (12, 256, 256, 14_375)],
                         ids=["64x64x172500", "256x64x172500", "12x256x256x14375"])
def test_at_size_against_the_restatement(shape):
    from sparse_rcnn_amd import evaluation as E
    b, p, g, n = shape
    rng = np.random.default_rng(p + g + n)
    masks = [_at_size_masks(rng, p, g, n) for _ in range(b)]
    assert n % 32
    pp, gp = packed([m[0] for m in masks], E), packed([m[1] for m in masks], E)
    for ps in pp + gp:                                           # both inputs: nothing beyond N in the last word
        assert int((ps.words[:, -1].to(torch.int64) & 0xFFFFFFFF).max()) < (1 << (n % 32))
    r, r2 = E.mask_iou(pp, gp), E.mask_iou(pp, gp)
    for t in ("inter", "pred_count", "gt_count"):
        assert torch.equal(getattr(r, t), getattr(r2, t))
    assert torch.equal(r.iou.view(torch.int32), r2.iou.view(torch.int32))
    k, thresholds = 18, [0.25, 0.5]
    score = [np.sort(rng.uniform(0, 1, p).astype(np.float32))[::-1].copy() for _ in range(b)]
    pcls = [rng.integers(0, k, p).astype(np.int64) for _ in range(b)]
    gcls = [pc[:g][np.arange(g) % p].copy() for pc in pcls]      # ground truth i has prediction i's class
    keep = [sc >= np.float32(0.2) for sc in score]
    recs = []
    for s in range(b):
        inter, pc, gc = ER.mask_counts(*masks[s])
        got = r.sample(s)
        assert same(got["inter"], inter.astype(np.int32)) and same(got["pred_count"], pc.astype(np.int32))
        assert same(got["gt_count"], gc.astype(np.int32)) and same(got["iou"], ER.iou_from_counts(inter, pc, gc))
        recs.append(dict(score=score[s], iou=ER.iou_from_counts(inter, pc, gc), keep=keep[s], pred_class=pcls[s], gt_class=gcls[s]))
    args = ([r.sample(s)["iou"] for s in range(b)], thresholds, [T(x) for x in keep], [T(x) for x in pcls], [T(x) for x in gcls], range(k))
    flags, num_gt = E.match(*args)                               # (1 + 18) x 2 x b problems, one launch
    flags2, _ = E.match(*args)
    assert torch.equal(flags, flags2)
    f, n_tp = flags.cpu().numpy(), 0
    for ci, c in enumerate([None] + list(range(k))):
        for ti, t in enumerate(thresholds):
            want = [ER.problem(rec, t, c) for rec in recs]
            got = f[ci, ti]
            assert np.array_equal(got[got >= 0] > 0, np.concatenate([w[1] for w in want])), (c, t)
            assert np.array_equal(num_gt[ci, ti].cpu().numpy(), [w[2] for w in want])
            n_tp += int((got > 0).sum())
    assert n_tp > 0 and (f[0] == 0).any()
    print(f"{shape}: {n_tp} true positives over {f.shape[0] * f.shape[1] * b} problems")


# ---- 5. edge cases -------------------------------------------------------------------------------------------------------------
def test_edge_cases():
    import sparse_rcnn_amd as scn
    from sparse_rcnn_amd import evaluation as E
    calc = E.MaskOverlapCalculator(0.5, score_threshold=0.5)
    gt = torch.zeros((3, 100), dtype=torch.bool, device=DEV)
    gt[0, :50] = True
    for p, g, n in ((0, 3, 100), (4, 0, 100), (4, 3, 0), (0, 0, 0)):
        acc = E.OverlapAccumulator(calc)
        acc.add_sample(torch.full((p,), 0.9, device=DEV), torch.full((p, n), 0.75, device=DEV), gt[:g, :n],
                       torch.zeros(p, dtype=torch.int64, device=DEV), torch.zeros(g, dtype=torch.int64, device=DEV))
        assert tuple(acc.records[0]["iou"].shape) == (p, g)
        c = acc.get_pr_curve(0.5)
        assert len(c.precision) == p and c.num_gt == g and not c.tp_indicator.any()
        ap = c.get_ap_interpolated_all_points()
        assert (np.isnan(ap.item()) if g == 0 else ap.item() == 0)      # (0 / 0 recall without ground truth, as the reference)
        col = acc.get_classwise_accumulator([0, 1]).get_pr_collection(0.5)
        assert [x.num_gt for x in col] == [g, 0]
        if n == 0 and p and g:
            assert torch.isnan(acc.records[0]["iou"]).all()
    boxes = E.bbox_iou([torch.zeros((0, 2, 3), device=DEV)], [torch.zeros((2, 2, 3), device=DEV)])
    assert tuple(boxes[0].shape) == (0, 2)
    conf = E.ConfusionAccumulator(E.ConfusionCalculator(20))
    conf.add_batch(torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV))
    assert not conf.get_confusion_matrix().confusion_matrix.any()
    conf.add_batch(T(np.array([1, 25, 3, 99], np.int64)), T(np.array([1, 2, -100, 20], np.int64)))   # one bad row: pred 25, gt 2
    with pytest.raises(scn.ScnError, match="1 rows"):
        conf.get_confusion_matrix()
    assert conf.confusion_list[-1].sum().item() == 1
    for bad in (lambda: E.bbox_iou([torch.zeros(1, 2, 3)], [torch.zeros(1, 2, 3)]),
                lambda: E.ConfusionCalculator(20)(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)),
                lambda: calc(torch.ones(1), torch.ones(1, 8), torch.ones(1, 8, dtype=torch.bool), None),
                lambda: E.match([torch.zeros(1, 1)], [0.5])):
        with pytest.raises(scn.ScnError, match="there is no CPU path"):
            bad()


# ---- 4. SceneStep.evaluate -----------------------------------------------------------------------------------------------------
def _same_outputs(a, b):
    assert set(a) == set(b)
    for key in a:
        for x, y in zip(a[key] if isinstance(a[key], (list, tuple)) else [a[key]], b[key] if isinstance(b[key], (list, tuple)) else [b[key]]):
            assert x.shape == y.shape and torch.equal(x.view(torch.uint8) if x.is_floating_point() else x,
                                                      y.view(torch.uint8) if y.is_floating_point() else y), key


@pytest.mark.parametrize("workload,n_gt", [("cfg3-rpn", None), ("ref-crop-rpn", 8)])
def test_scene_step_evaluate(workload, n_gt):
    """evaluate(score_threshold = the median roi_score: a freshly initialised RPN scores near 0.5, the reference's 0.9 would keep
    nothing) against the restated evaluation fed from predict()'s DENSE outputs and the scene's ground truth: `bbox`, `mask` and
    `segment` completely (IoU matrices and flags equal, metrics within n * 2^-24); the ground-truth-box metrics (`gtbbox`,
    `gtmask`, `gtlabelmask`, which predict() does not output) restated from the accumulators' overlap matrices and the binary
    confusion tensors.  predict() before and after evaluate() is bit-identical."""
    import sparse_rcnn_amd as scn
    from sparse_rcnn_amd.trainstep import SceneStep
    with pytest.raises(ValueError, match="class_loss=True"):
        SceneStep("cfg3-rpn", prefetch=False).evaluate()
    kw = {} if n_gt is None else dict(n_gt=n_gt)
    st = SceneStep(workload, optimizer="adam", rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True,
                   prefetch=False, lr=1e-4, **kw)
    for _ in range(3):
        st.step()
    st.finish()
    before = st.predict()
    st.finish()
    st.evaluate(score_threshold=0.0)
    st.finish()
    scores = torch.cat([r["score"] for r in st.eval_out["overlap"]["bbox"].records])
    t = float(scores.median().item())
    thresholds = (0.25, 0.5)
    combined, single_class = st.evaluate(score_threshold=t)
    st.finish()
    after = st.predict()
    st.finish()
    _same_outputs(before, after)
    acc = st.eval_out["overlap"]
    sc = st._scenes[0]
    b = len(before["roi_bbox"])
    assert set(acc) == set(ER.OVERLAP_NAMES) and all(len(a.records) == b for a in acc.values())
    recs = {n: [] for n in ER.OVERLAP_NAMES}
    for s in range(b):
        score = acc["bbox"].records[s]["score"].cpu().numpy()
        keep = score >= np.float32(t)
        pcls, labels = before["class"][s].cpu().numpy(), sc["gt_label"][s].cpu().numpy()
        pred, gt = (before["mask"][s] > 0.5).cpu().numpy(), sc["gt_mask_cpu"][s].numpy().astype(bool)
        boxes = ER.box_iou(before["roi_bbox"][s].cpu().numpy(), sc["gt_dev"][s].cpu().numpy().reshape(-1, 2, 3))
        recs["bbox"].append(dict(score=score, iou=boxes, keep=keep, pred_class=pcls, gt_class=labels))
        recs["mask"].append(dict(score=score, iou=ER.mask_iou(pred, gt), keep=keep, pred_class=pcls, gt_class=labels))
        for n in ("bbox", "mask"):
            assert same(acc[n].records[s]["iou"], recs[n][-1]["iou"]), (n, s)
            assert same(acc[n].records[s]["pred_class"], pcls) and same(acc[n].records[s]["keep"].bool(), keep)
        for n in ("gtbbox", "gtmask", "gtlabelmask"):
            r = acc[n].records[s]
            recs[n].append({key: (None if v is None else v.cpu().numpy()) for key, v in r.items()})
            assert same(r["gt_class"], labels) and r["iou"].shape == (len(labels), len(labels))
        assert same(acc["gtbbox"].records[s]["iou"], ER.box_iou(sc["gt_dev"][s].cpu().numpy().reshape(-1, 2, 3),
                                                               sc["gt_dev"][s].cpu().numpy().reshape(-1, 2, 3)))
    k = 18
    for n in ("bbox", "mask"):
        flags, _ = scn.evaluation.match([r["iou"] for r in acc[n].records], thresholds, [r["keep"] for r in acc[n].records])
        f = flags.cpu().numpy()
        tp = np.stack([np.concatenate([ER.problem(r, t)[1] for r in recs[n]]) for t in thresholds])
        assert np.array_equal(np.stack([f[0, i][f[0, i] >= 0] > 0 for i in range(2)]), tp), n
    seg = ER.confusion(before["segmentation_class"].cpu().numpy(), sc["seg_target"].cpu().numpy(), 20)
    assert np.array_equal(st.eval_out["confusion"]["segment"].confusion_matrix, seg)
    labels_all = np.concatenate([l.cpu().numpy() for l in sc["gt_label"]])
    gt_class = np.concatenate([r["pred_class"] for r in recs["gtbbox"]])
    label_conf = ER.confusion(gt_class, labels_all, k)
    assert np.array_equal(st.eval_out["overlap_confusion"]["gtbbox"].confusion_matrix, label_conf)
    bin_conf = torch.cat(st.eval_out["gtlabelmask"].confusion_matrix_list).cpu().numpy()
    for s in range(b):                                           # tp / (tp + fp + fn) of pair i is the overlap matrix's diagonal
        c = st.eval_out["gtlabelmask"].confusion_matrix_list[s].cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            d = c[:, 0, 0].astype(np.float32) / (c[:, 0, 0] + c[:, 0, 1] + c[:, 1, 0]).astype(np.float32)
        assert np.array_equal(d, np.diagonal(recs["gtlabelmask"][s]["iou"]), equal_nan=True)
        assert (c.sum((1, 2)) == st.splits[s]).all()
    want = ER.metrics(recs, {"segment": seg}, {"gtbbox": label_conf}, {"gtlabelmask": (bin_conf, labels_all)}, list(thresholds),
                      list(range(k)), list(range(k)), (None, 11), list(range(20)))
    want_combined = {key: v for key, v in want[0].items() if "gtbbox_AP" not in key}
    n_curve = max(max(want[2].values()), 20)
    worst = ER.compare_metrics((combined, single_class), (want_combined, want[1]), ER.ap_bound(n_curve), workload)
    kept = int(sum(r["keep"].sum() for r in recs["mask"]))
    print(f"{workload}: threshold {t:.4f} keeps {kept} of {len(scores)}; mask_AP_0.25 {combined['mask_AP_0.25']:.4f} "
          f"bbox_AP_0.25 {combined['bbox_AP_0.25']:.4f} segment_avg_iou {combined['segment_avg_iou']:.4f}; worst metric "
          f"difference {worst:.3e} (bound {ER.ap_bound(n_curve):.3e})")
    assert 0 < kept < len(scores)


def test_forward_only_and_predict_share_their_chain():
    """forward_only() and predict() run one inference chain (SceneStep._infer): the same backbone, RPN, selection and boxes --
    cfg3-rpn cuts nothing off its proposals (`mask_boxes` None) -- so the mask logits of the two are the same bits."""
    from sparse_rcnn_amd.trainstep import SceneStep
    st = SceneStep("cfg3-rpn", target=10_000, grid=(128, 128, 64), n_gt=4, class_loss=True, prefetch=False)
    assert st.mask_boxes is None
    _, logits = st.forward_only(0)
    st.predict(0)
    assert logits.shape[0] > 0 and logits.shape == st.predict_out[1].shape
    assert torch.equal(logits, st.predict_out[1])
