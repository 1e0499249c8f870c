"""CPU: the restatement of the RPN loss path (tests/rpnloss_restate.py) reproduces the reference's own outputs
(tests/golden/rpn_loss_*.npz, made by tests/golden/make_rpn_loss_golden.py), and sparse_rcnn_amd.loss refuses what it does not
compute."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rpnloss_restate as RS                                   # noqa: E402

CASES = sorted(glob.glob(os.path.join(HERE, "golden", "rpn_loss_*.npz")))


def test_fixtures_present():
    names = {os.path.basename(p)[9:-4] for p in CASES}
    assert {"one_level", "two_levels", "empty_sample", "pos_gt_neg", "pos_eq_neg", "no_negatives"} <= names
    for p in CASES:
        assert os.path.getsize(p) <= 200 * 1024


@pytest.mark.parametrize("path", CASES, ids=lambda p: os.path.basename(p)[9:-4])
def test_restatement_reproduces_reference(path):
    z = np.load(path)
    ov, am, tg = RS.targets(z["inside_anchors"], z["gt_boxes"], z["gt_offsets"])
    assert np.array_equal(ov.view(np.int32), z["max_overlaps"].view(np.int32))
    assert np.array_equal(am, z["argmax"])
    assert RS.ulp_diff(tg, z["bbox_targets"]).max() <= 2
    # the draw of the fixture: the members of the larger set that carry a score weight
    ovr = z["max_overlaps"]
    pos, neg = ovr >= np.float32(0.35), ovr < np.float32(0.15)
    larger = pos if pos.sum() > neg.sum() else neg
    drawn = larger & (z["score_weight"] > 0)
    assert drawn.sum() == min(pos.sum(), neg.sum())
    labels, sw, bw = RS.weights_for(ovr, drawn)
    for got, name in ((labels, "labels"), (sw, "score_weight"), (bw, "bbox_weights")):
        assert np.array_equal(got, z[name]), name
    sl, bl, ds, db = RS.loss(z["rpn_score"], z["rpn_bbox"], z["labels"], z["score_weight"], z["bbox_targets"],
                             z["bbox_weights"])
    for got, ref in ((sl, z["score_loss"]), (bl, z["bbox_loss"])):
        assert abs(got - float(ref)) <= 1e-6 * max(abs(float(ref)), 1e-30) or got == float(ref) == 0.0
    assert RS.close_grad(ds, z["grad_score"])
    assert RS.close_grad(db, z["grad_bbox"])


def test_empty_sample_fixture_has_the_reference_else_branch():
    z = np.load(os.path.join(HERE, "golden", "rpn_loss_empty_sample.npz"))
    assert z["gt_offsets"][1] == z["gt_offsets"][2]
    assert (z["max_overlaps"][1] == 0).all() and (z["argmax"][1] == -1).all()


def test_refusals_without_gpu():
    from sparse_rcnn_amd import loss as RL
    with pytest.raises(ValueError):
        RL.SamplewiseBboxTargetSelector()
    with pytest.raises(ValueError):
        RL.BatchwiseBboxTargetSelector(0.1, 0.2)
    with pytest.raises(ValueError):
        RL.RpnLoss(RL.BatchwiseBboxTargetSelector(), sigma=0.0)
    with pytest.raises(RL.L.ScnError):                       # CPU anchors: no CPU path
        RL.rpn_target_calculator(torch.zeros(4, 2, 3))
    with pytest.raises((ValueError, RL.L.ScnError)):
        RL.rpn_target_calculator(torch.zeros(4, 2, 3, dtype=torch.float64))
    with pytest.raises(RL.L.ScnError):
        RL.BatchwiseBboxTargetSelector()(torch.zeros(2, 4))
    with pytest.raises(RL.L.ScnError):
        RL.RpnLoss(RL.BatchwiseBboxTargetSelector()).loss((None,) * 3 + (torch.zeros(1, 4),) * 3, torch.zeros(1, 4),
                                                          torch.zeros(1, 4, 2, 3))


def test_selector_state_dict_round_trip():
    from sparse_rcnn_amd import loss as RL
    a = RL.BatchwiseBboxTargetSelector(seed=5)
    a.counter = 17
    b = RL.BatchwiseBboxTargetSelector(seed=0)
    b.load_state_dict(a.state_dict())
    assert (b.seed, b.counter) == (5, 17)
    crit = RL.RpnLoss(a)
    assert crit.state_dict()["bbox_target_selector._extra_state"] == {"seed": 5, "counter": 17}


def test_scenestep_refuses_rpn_loss_without_rpn():
    from sparse_rcnn_amd.trainstep import SceneStep
    with pytest.raises(ValueError):
        SceneStep("cfg3", device=torch.device("cpu"), rpn_loss=True)
