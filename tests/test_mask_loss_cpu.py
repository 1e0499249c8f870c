"""CPU: the restatement of the mask-training path (tests/maskloss_restate.py) reproduces the reference's own outputs
(tests/golden/mask_loss_*.npz, made by tests/golden/make_mask_loss_golden.py); synthetic instances are deterministic and lie
inside their boxes' crops; the packed-mask layout round-trips; sparse_rcnn_amd.loss refuses what it does not compute."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import maskloss_restate as MS                                  # noqa: E402
import rpnloss_restate as RS                                   # noqa: E402

CASES = sorted(glob.glob(os.path.join(HERE, "golden", "mask_loss_*.npz")))


def _ids(p):
    return os.path.basename(p)[10:-4]


def test_fixtures_present():
    assert {_ids(p) for p in CASES} >= {"basic", "weights", "empty"}
    for p in CASES:
        assert os.path.getsize(p) <= 200 * 1024


@pytest.mark.parametrize("path", CASES, ids=_ids)
def test_restatement_reproduces_overlaps(path):
    z = np.load(path)
    preds, gts, _, _ = MS.fixture(z)
    mx, am = zip(*(MS.overlap(p, g) for p, g in zip(preds, gts)))
    assert np.array_equal(np.concatenate(mx).view(np.int32), z["max_overlap"].view(np.int32))
    assert np.array_equal(np.concatenate(am), z["argmax"])


@pytest.mark.parametrize("path", CASES, ids=_ids)
def test_fixture_selection_is_the_reference_rule(path):
    """The recorded draw: min(24, #positives) distinct positives per sample, then every ground truth in order."""
    z = np.load(path)
    preds, gts, _, _ = MS.fixture(z)
    o = d = f = 0
    for s, (p, g) in enumerate(zip(preds, gts)):
        mx = z["max_overlap"][o:o + len(p)]
        nd = int(z["drawn_counts"][s])
        drawn = z["drawn"][d:d + nd]
        assert nd == min(24, int((mx >= np.float32(0.2)).sum()))
        assert len(set(drawn.tolist())) == nd and (mx[drawn] >= np.float32(0.2)).all()
        fwd = z["fwd_boxes"][f:f + nd + len(g)]
        assert np.array_equal(fwd[:nd], p[drawn]) and np.array_equal(fwd[nd:], g)
        assoc = z["gt_association"][f:f + nd + len(g)]
        assert np.array_equal(assoc[:nd], z["argmax"][o:o + len(p)][drawn]) and np.array_equal(assoc[nd:], np.arange(len(g)))
        o, d, f = o + len(p), d + nd, f + nd + len(g)


@pytest.mark.parametrize("path", CASES, ids=_ids)
def test_restatement_reproduces_inside_loss_and_gradient(path):
    z = np.load(path)
    _, _, labels, masks = MS.fixture(z)
    counts = z["fwd_counts"]
    sample = np.repeat(np.arange(len(counts)), counts)
    ins = MS.inside(z["coords"], z["fwd_boxes"], sample)
    assert np.array_equal(ins, MS.fixture_inside(z))
    splits = [int(z["n_pts"])] * len(counts)
    l, g = MS.loss(z["scores"], ins, counts, splits, z["gt_association"], z["gt_labels"], z["gt_counts"], masks,
                   z["class_weights"])
    ref = float(z["loss"])
    assert abs(l - ref) <= 1e-6 * abs(ref), (l, ref)
    rel = np.linalg.norm(g.astype(np.float64) - z["grad"]) / np.linalg.norm(z["grad"])
    assert rel <= 1e-6, rel


def test_empty_fixture_drops_boxes_without_points():
    z = np.load(os.path.join(HERE, "golden", "mask_loss_empty.npz"))
    assert (z["box_rows"] == 0).any() and z["gt_counts"].min() == 0


def test_make_instances_deterministic_and_inside_the_crop():
    from sparse_rcnn_amd.synthetic import make_batch, make_boxes, make_instances
    coords, _, _, _, splits = make_batch(2, (64, 64, 32), 3000, seed=3)
    boxes = make_boxes(coords, 12, seed=4, lo=4.0, hi=24.0)
    l1, m1 = make_instances(coords, boxes, n_classes=18, seed=9)
    l2, m2 = make_instances(coords, boxes, n_classes=18, seed=9)
    c = coords.numpy()
    some_partial = False
    for s in range(2):
        assert torch.equal(l1[s], l2[s]) and torch.equal(m1[s], m2[s])
        assert l1[s].dtype == torch.int64 and l1[s].shape == (12,) and int(l1[s].min()) >= 0 and int(l1[s].max()) < 18
        assert m1[s].dtype == torch.bool and m1[s].shape == (12, splits[s])
        pts = c[c[:, 3] == s]
        crop = MS.inside(pts, boxes[s].numpy(), np.full(12, s))
        m = m1[s].numpy()
        assert not (m & ~crop).any()                                   # a subset of each box's crop
        some_partial |= bool(((m.sum(1) > 0) & (m.sum(1) < crop.sum(1))).any())
    assert some_partial                                                # some, not all, of a box's points
    l3, _ = make_instances(coords, boxes, n_classes=18, seed=10)
    assert not all(torch.equal(a, b) for a, b in zip(l1, l3))


def test_pack_layout_round_trips():
    g = np.random.default_rng(0)
    for n in (1, 31, 32, 33, 100, 257):
        m = g.uniform(0, 1, (5, n)) < 0.3
        w = MS.pack(m)
        assert w.shape == (5, (n + 31) // 32) and w.dtype == np.uint32
        assert np.array_equal(MS.unpack(w, n), m)
        assert int(w[0, 0]) & 1 == int(m[0, 0])                        # point 0 = bit 0 of word 0


def test_refusals():
    from sparse_rcnn_amd import ScnError
    from sparse_rcnn_amd.loss import MaskLoss, OverlapCalculator, TrainSelector, pack_gt_masks
    with pytest.raises(ValueError):
        TrainSelector(0.2, negative_threshold=0.1)
    with pytest.raises(ValueError):
        TrainSelector(0.2, 0, random_selector=(24, 4, True))
    with pytest.raises(ValueError):
        TrainSelector(0.2, 0, random_selector=None)
    sel = TrainSelector(0.2)
    assert sel.num_pos == 24 and sel.get_extra_state()["counter"] == 0
    cpu_boxes = [torch.zeros((3, 2, 3))]
    with pytest.raises(ScnError):
        OverlapCalculator()(cpu_boxes, cpu_boxes)
    with pytest.raises(ScnError):
        sel.select(cpu_boxes, cpu_boxes)
    with pytest.raises(ScnError):
        sel([(cpu_boxes[0], cpu_boxes[0], torch.zeros(3), torch.zeros(3, dtype=torch.long))])
    with pytest.raises(ScnError):
        pack_gt_masks([torch.zeros((2, 5), dtype=torch.bool)])
    with pytest.raises((ValueError, ScnError)):
        MaskLoss()(torch.zeros((4, 18), dtype=torch.float64), None, [], [], [])
    with pytest.raises(ScnError):
        MaskLoss()(torch.zeros((4, 18)), None, [], [], [])


def test_scenestep_refuses_mask_loss_without_rpn():
    from sparse_rcnn_amd.trainstep import SceneStep
    for wl in ("cfg2", "cfg3", "ref-crop"):
        with pytest.raises(ValueError):
            SceneStep(wl, mask_loss=True)
        with pytest.raises(ValueError):
            SceneStep(wl, n_gt=8)
