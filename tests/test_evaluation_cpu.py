"""CPU: the numpy restatement of the evaluation (tests/eval_restate.py) reproduces every fixture the reference wrote
(tests/golden/eval_*.npz): IoU matrices, true-positive flags and count matrices exactly, curve values and metrics within
n * 2^-24 for a curve of n points (the restatement's curve is float64, the reference's fp32: the same bound the device is
held to).  The at-size GPU tests rely on this restatement, since the reference does not travel with the repository.  Also
the host side of sparse_rcnn_amd.evaluation that needs no GPU: the curve arithmetic and the refusal of CPU tensors."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eval_restate as ER                                      # noqa: E402

CASES = sorted(glob.glob(os.path.join(HERE, "golden", "eval_*.npz")))


def _id(p):
    return os.path.basename(p)[5:-4]


def test_fixtures_exist_and_are_small():
    assert {_id(p) for p in CASES} >= {"basic", "empty", "nan", "ties_iou", "boxes"}
    assert all(os.path.getsize(p) < 100_000 for p in CASES)


@pytest.mark.parametrize("path", CASES, ids=_id)
def test_restatement_reproduces_overlaps_flags_and_counts(path):
    z, samples = ER.load_case(path)
    recs = ER.case_records(z, samples)
    for s, d in enumerate(samples):
        for key, rec in (("mask_iou", recs["mask"]), ("box_iou", recs["bbox"]), ("gtmask_iou", recs["gtmask"])):
            got, want = rec[s]["iou"], z[f"{key}_{s}"]
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.array_equal(got, want, equal_nan=True), (key, s)
    thresholds = [float(t) for t in z["thresholds"]]
    for n in ER.OVERLAP_NAMES:
        tp, tpc, num_gt = ER.case_flags(recs[n], thresholds, range(int(z["k"])))
        assert np.array_equal(tp, z[f"tp_{n}"]) and np.array_equal(tpc, z[f"tpc_{n}"]), n
        assert np.array_equal(num_gt, z[f"class_num_gt_{n}"]), n
        assert np.array_equal([int(r["keep"].sum()) for r in recs[n]], z[f"kept_{n}"]), n
    _, _, _, conf = ER.case_metrics(z, samples, recs)
    assert np.array_equal(conf["segment"], z["segment_confusion"])
    assert np.array_equal(conf["gtbbox"], z["gtbbox_confusion"])
    assert np.array_equal(conf["gtlabelmask"], z["gtlabelmask_confusion"])
    labels = np.concatenate([s["labels"] for s in samples])
    mats, _, _, mean_iou, _ = ER.binary_collection(conf["gtlabelmask"], labels, range(int(z["k"])))
    assert np.array_equal(mats, z["gtlabelmask_classwise"])
    assert ER.same_nan(mean_iou, z["gtlabelmask_classwise_mean_iou"])
    assert ER.max_diff(mean_iou, z["gtlabelmask_classwise_mean_iou"]) <= ER.ap_bound(len(labels))


@pytest.mark.parametrize("path", CASES, ids=_id)
def test_restatement_reproduces_curves_and_metrics(path):
    z, samples = ER.load_case(path)
    recs = ER.case_records(z, samples)
    worst = 0.0
    for n in ER.OVERLAP_NAMES:
        for t in (float(t) for t in z["single_thresholds"]):
            c = ER.Curve(recs[n], t)
            assert np.array_equal(c.score, z[f"curve_{n}_{t}_score"]) and np.array_equal(c.tp_indicator, z[f"curve_{n}_{t}_tp"])
            assert c.num_gt == int(z[f"curve_{n}_{t}_num_gt"])
            for got, key in ((c.precision, "precision"), (c.recall, "recall"), (c.precision_interpolated, "interpolated")):
                want = z[f"curve_{n}_{t}_{key}"]
                assert np.array_equal(got.astype(np.float32), want, equal_nan=True), (n, t, key)   # one division each
    combined, single_class, n_points, _ = ER.case_metrics(z, samples, recs)
    bound = ER.ap_bound(max(max(n_points.values()), int(z["seg"])))      # (the longest curve; a mean over the 20 segmentation classes)
    worst = ER.compare_metrics((combined, single_class), ER.expected_metrics(z), bound, _id(path))
    print(f"{_id(path)}: worst metric difference {worst:.3e} (bound {bound:.3e})")


def test_fixtures_are_not_degenerate():
    z, _ = ER.load_case(os.path.join(HERE, "golden", "eval_basic.npz"))
    i05 = [float(t) for t in z["thresholds"]].index(0.5)
    tp = z["tp_mask"][i05]
    assert tp.any() and not tp.all()
    kept, total = int(z["kept_mask"].sum()), int(z["n_pred"].sum())
    assert kept < total <= 2 * kept
    cap = ER.expected_metrics(z)[1]["mask_class_AP_0.5"]
    vals = np.array(list(cap.values()))
    assert (vals == 0).any() and np.isnan(vals).any() and (vals > 0).any()
    zn, _ = ER.load_case(os.path.join(HERE, "golden", "eval_nan.npz"))
    assert np.isnan(zn["mask_iou_0"][0, 0])
    zt, _ = ER.load_case(os.path.join(HERE, "golden", "eval_ties_iou.npz"))
    assert zt["mask_iou_0"][0, 0] == zt["mask_iou_0"][0, 1]


def test_matching_restated_nan_and_tie_rules():
    z = np.load(os.path.join(HERE, "golden", "eval_nan.npz"))      # hand-written matrices, flags by the reference's own loop
    for i in range(2):
        got = np.stack([ER.match(z[f"rule_iou_{i}"], float(t)) for t in z["thresholds"]])
        assert np.array_equal(got, z[f"rule_tp_{i}"]), i
    assert np.isnan(z["rule_iou_1"][0, 0]) and z["rule_iou_1"][0, 1] >= 0.5 and not z["rule_tp_1"][:, 0].any()
    assert ER.match(np.array([[np.nan, .9], [.8, .7]], np.float32), 0.5).tolist() == [False, True]
    assert ER.match(np.array([[.6, .6], [.6, .1]], np.float32), 0.5).tolist() == [True, False]     # first index wins the tie
    assert ER.match(np.zeros((3, 0), np.float32), 0.5).tolist() == [False] * 3


@pytest.mark.parametrize("path", CASES, ids=_id)
def test_package_curve_arithmetic_matches_fixture(path):
    """sparse_rcnn_amd.evaluation.PrecisionRecallCurve (torch, host side) on the fixture's sorted flags: precision, recall and
    the interpolated precision bit-equal, AP within n * 2^-24 of the reference's own value."""
    from sparse_rcnn_amd.evaluation import PrecisionRecallCurve, average_precision, metric_key
    z, _ = ER.load_case(path)
    want = ER.expected_metrics(z)[0]
    for n in ER.OVERLAP_NAMES:
        for t in (float(t) for t in z["single_thresholds"]):
            c = PrecisionRecallCurve(torch.from_numpy(z[f"curve_{n}_{t}_score"]), torch.from_numpy(z[f"curve_{n}_{t}_tp"]),
                                     int(z[f"curve_{n}_{t}_num_gt"]))
            assert np.array_equal(c.precision.numpy(), z[f"curve_{n}_{t}_precision"], equal_nan=True)
            assert np.array_equal(c.recall.numpy(), z[f"curve_{n}_{t}_recall"], equal_nan=True)
            assert np.array_equal(c.precision_interpolated.numpy(), z[f"curve_{n}_{t}_interpolated"], equal_nan=True)
            if n == "gtbbox":
                continue                                          # (its AP keys are dropped, training.py:174-177)
            for method in (None, 11):
                key = metric_key(n, "AP", t, method)
                got = average_precision(c, method).item()
                assert ER.same_nan(got, want[key]) and ER.max_diff(got, want[key]) <= ER.ap_bound(len(c.recall)), (key, got)


def test_helper_key_strings_and_default_names():
    from sparse_rcnn_amd.evaluation import EvaluationHelper, metric_key
    assert metric_key("mask", "AP", 0.5, None) == "mask_AP_0.5"
    assert metric_key("mask", "mAP", 0.25, 11) == "mask_mAP_0.25_{method}_points"
    h = EvaluationHelper([0.25, 0.5, ("[0.5:0.95:0.05]", (0.5, 0.75))], range(18))
    assert h.overlap_thresholds == [0.25, 0.5, 0.75] and h.overlap_class_names[7] == 7
    assert h({}, {}, {}, {})[:2] == ({}, {})


def test_cpu_tensors_are_refused():
    import sparse_rcnn_amd as scn
    from sparse_rcnn_amd import evaluation as E
    with pytest.raises(scn.ScnError, match="there is no CPU path"):
        E.BboxOverlapCalculator()(torch.ones(2), torch.zeros(2, 2, 3), torch.zeros(1, 2, 3), None)
    with pytest.raises(scn.ScnError, match="there is no CPU path"):
        E.ConfusionCalculator(20)(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(scn.ScnError, match="there is no CPU path"):
        E.MaskOverlapCalculator()(torch.ones(2), torch.zeros(2, 40), torch.zeros(1, 40, dtype=torch.bool), None)


class _RestatedOverlaps:
    """Stands in for an OverlapAccumulator whose matching ran on the device: the sorted flags come from the restatement."""

    def __init__(self, records):
        self.records = records

    def has_classes(self):
        return True

    def matched(self, thresholds, classes=None):
        out = {}
        for c in [None] + list(classes or []):
            for t in thresholds:
                cur = ER.Curve(self.records, t, c)
                out[(c, float(t))] = (torch.from_numpy(cur.score.astype(np.float32)), torch.from_numpy(cur.tp_indicator), cur.num_gt)
        return out


@pytest.mark.parametrize("path", CASES, ids=_id)
def test_package_helper_and_confusion_classes_match_fixture(path):
    """Everything of sparse_rcnn_amd.evaluation behind the kernels -- EvaluationHelper, the curves, ConfusionMatrix,
    BinaryConfusionMatrixCollection -- on host tensors: the reference's metric dictionaries, key for key, within n * 2^-24."""
    from sparse_rcnn_amd import evaluation as E
    z, samples = ER.load_case(path)
    recs = ER.case_records(z, samples)
    _, _, n_points, conf = ER.case_metrics(z, samples, recs)
    labels = np.concatenate([s["labels"] for s in samples])
    k = int(z["k"])

    class Conf:
        def __init__(self, m):
            self.m = m

        def get_confusion_matrix(self, device=None):
            return E.ConfusionMatrix(torch.from_numpy(self.m))

    class Binary:
        def get_binary_confusion_matrix_collection(self, classes, device=None):
            return E.BinaryConfusionMatrixCollection(torch.from_numpy(conf["gtlabelmask"]), torch.from_numpy(labels), classes)

    helper = E.EvaluationHelper(ER.thresholds_of(z), list(range(k)), [str(x) for x in z["class_names"]], [None, 11],
                                [str(x) for x in z["seg_names"]])
    combined, single_class, _, cm, ocm, binary = helper({n: _RestatedOverlaps(recs[n]) for n in ER.OVERLAP_NAMES},
                                                        {"segment": Conf(conf["segment"])}, {"gtbbox": Conf(conf["gtbbox"])},
                                                        {"gtlabelmask": Binary()})
    combined = {key: v for key, v in combined.items() if "gtbbox_AP" not in key}
    bound = ER.ap_bound(max(max(n_points.values()), int(z["seg"])))
    worst = ER.compare_metrics((combined, single_class), ER.expected_metrics(z), bound, _id(path))
    assert np.array_equal(binary["gtlabelmask"].classwise_confusion_matrices, z["gtlabelmask_classwise"])
    assert ER.same_nan(binary["gtlabelmask"].classwise_mean_iou, z["gtlabelmask_classwise_mean_iou"])
    assert ER.max_diff(binary["gtlabelmask"].classwise_mean_iou, z["gtlabelmask_classwise_mean_iou"]) <= ER.ap_bound(len(labels))
    assert np.array_equal(cm["segment"].confusion_matrix, z["segment_confusion"])
    print(f"{_id(path)}: worst metric difference {worst:.3e} (bound {bound:.3e})")
