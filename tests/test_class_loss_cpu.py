"""CPU: the float64 restatement of the class / segmentation loss path (tests/xent_restate.py) reproduces the reference's own
outputs (tests/golden/class_loss_*.npz, xent_*.npz, made by tests/golden/make_class_golden.py); the class branch and the
segmentation head carry the reference's parameters under the reference's names (dropin_class_network.json); synthetic
segmentation labels; SceneStep refuses what it documents; the step model's defaults are what they were
(stepmodel_params.json, written before the class branch existed).

Bounds: 1e-6 relative on the loss, 1e-6 relative L2 on the gradient, 1e-6 absolute on probabilities -- the bound of the RPN-
and mask-loss tests.  torch's fp32 cross_entropy on the CPU sits at most 1.8e-7 (loss) and 9.4e-8 (gradient) from its own
float64 evaluation for n from 56 to 600 000, c 18 / 20, logit scales 1 and 8, weights and 20 % ignored rows."""
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import xent_restate as XR                                      # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
XENT = sorted(glob.glob(os.path.join(GOLDEN, "xent_*.npz")))
CLASS = sorted(glob.glob(os.path.join(GOLDEN, "class_loss_*.npz")))
TOL = 1e-6


def _xid(p):
    return os.path.basename(p)[5:-4]


def _cid(p):
    return os.path.basename(p)[11:-4]


def test_fixtures_present():
    assert len(XENT) == 9 and {_cid(p) for p in CLASS} == {"basic", "weights", "empty", "nodesc"}
    for p in XENT + CLASS:
        assert os.path.getsize(p) < 100 * 1024
    shapes = {(int(np.load(p)["n"]), int(np.load(p)["c"])) for p in XENT}
    assert shapes == {(300, 18), (4000, 20)}
    assert sum(int(np.load(p)["tie"]) for p in XENT) == 1


@pytest.mark.parametrize("path", XENT, ids=_xid)
def test_restatement_meets_cross_entropy(path):
    z = np.load(path)
    x = XR.fixture_logits(z)
    step = int(z["row_step"])
    loss, grad, n_bad = XR.cross_entropy(x, z["targets"], z["weights"])
    assert n_bad == 0
    ignored = float((z["targets"] == -100).mean())
    assert 0.1 < ignored < 0.3
    print(f"{_xid(path)}: loss {XR.rel(loss, z['loss']):.2e}  grad {XR.rel_l2(grad[::step], z['grad_rows']):.2e}")
    assert XR.rel(loss, z["loss"]) <= TOL
    assert XR.rel_l2(grad[::step], z["grad_rows"]) <= TOL
    assert XR.rel(np.sqrt((grad ** 2).sum()), z["grad_norm"]) <= TOL
    assert not grad[z["targets"] == -100].any()


@pytest.mark.parametrize("path", XENT, ids=_xid)
def test_restatement_meets_predictors(path):
    z = np.load(path)
    x = XR.fixture_logits(z)
    step = int(z["row_step"])
    idx = XR.argmax_first(x)
    assert np.array_equal(idx, z["seg_class"]) and np.array_equal(idx, z["class_indices"])
    assert np.abs(XR.softmax(x)[::step] - z["prob_rows"]).max() <= TOL
    if int(z["tie"]):
        assert x[5, 3] == x[5, 7] == x[5].max() and idx[5] == 3 and idx[9] == 0


@pytest.mark.parametrize("path", CLASS, ids=_cid)
def test_restatement_meets_class_loss(path):
    z = np.load(path)
    labels = XR.class_labels(z)
    full = np.concatenate(labels)
    assert np.array_equal(full, z["labels_full"])
    counts = z["box_counts"].tolist()
    valid = [int((l >= 0).sum()) for l in labels]
    assert valid == z["valid_counts"].tolist()
    # every sample but the one without ground truth in case (c) has a valid row
    assert all(v > 0 for v, c in zip(valid, counts) if c) and (min(counts) > 0 or _cid(path) == "empty")
    if int(z["nodesc"]):
        # the reference's compacted labels are the kept rows of the uncompacted ones; some rows fall between the thresholds
        assert np.array_equal(full[z["keep"]], z["labels"]) and (full[~z["keep"]] == -100).all()
        assert 0 < int((~z["keep"]).sum()) and (z["labels"] == int(z["negative_label"])).any()
    else:
        assert np.array_equal(full, z["labels"])
        assert (z["drawn_counts"] <= 32).all()
    loss, grad, n_bad = XR.cross_entropy(z["scores"], full, z["class_weights"])
    assert n_bad == 0
    print(f"{_cid(path)}: loss {XR.rel(loss, z['loss']):.2e}  grad {XR.rel_l2(grad, z['grad']):.2e}")
    assert XR.rel(loss, z["loss"]) <= TOL and XR.rel_l2(grad, z["grad"]) <= TOL


def test_fixture_basic_has_more_positives_than_slots():
    z = np.load(os.path.join(GOLDEN, "class_loss_basic.npz"))
    off = np.concatenate([[0], np.cumsum(z["pred_counts"])])
    npos = [int((z["max_overlap"][off[s]:off[s + 1]] >= 0.1).sum()) for s in range(2)]
    assert npos[0] > 32 > npos[1] > 0 and z["drawn_counts"].tolist() == [32, npos[1]]


def test_restatement_deviations():
    x = np.random.default_rng(0).standard_normal((6, 20))
    loss, grad, n_bad = XR.cross_entropy(x, np.full(6, -100))
    assert loss == 0.0 and not grad.any() and n_bad == 0
    t = np.array([1, 20, -5, -100, 3, 0])
    loss, grad, n_bad = XR.cross_entropy(x, t)
    ref, gref, _ = XR.cross_entropy(x[[0, 4, 5]], t[[0, 4, 5]])
    assert n_bad == 2 and loss == ref and np.array_equal(grad[[0, 4, 5]], gref) and not grad[[1, 2, 3]].any()


# ---- the branch and the head ---------------------------------------------------------------------------------------------
def _dropin():
    with open(os.path.join(GOLDEN, "dropin_class_network.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("fc", [256, 80])
def test_class_branch_carries_the_reference_parameters(fc):
    from sparse_rcnn_amd.classhead import ClassBranch
    fx = _dropin()[f"class_{fc}"]
    torch.manual_seed(0)
    br = ClassBranch(fc, 8)
    kmap, own = br.reference_key_map(), br.named_oracle_params()
    assert set(kmap) == set(fx["keys"]) and len(kmap) == 22
    assert set(kmap.values()) == set(own) and len(own) == len(list(br.parameters()))
    for rk, name in kmap.items():
        assert list(own[name].shape) == fx["keys"][rk], rk
    assert sum(p.numel() for p in br.parameters()) == fx["n_params"] == {256: 1261426, 80: 1255794}[fc]
    g = torch.Generator().manual_seed(3)
    sd = {"class_network." + k: torch.randn(shape, generator=g) for k, shape in fx["keys"].items()}
    sd["class_network.input_conv_layer.0.0.0.weight"] = sd["class_network.input_conv_layer.0.0.0.weight"].unsqueeze(1)
    sd["mask_network.input_conv_layer.0.0.0.weight"] = torch.zeros(1, fc, 16)          # (a sibling the detection must skip)
    missing, unused = br.load_reference_state_dict(sd)
    assert not missing and not unused
    for rk, name in kmap.items():
        assert torch.equal(own[name], sd["class_network." + rk].reshape(own[name].shape)), rk
    del sd["class_network.linear_layer.3.bias"]
    with pytest.raises(KeyError):
        br.load_reference_state_dict(sd, prefix="class_network.")
    assert fx["census"] == {"SubmanifoldConvolution": 7, "Convolution": 2, "ReLU": 6, "ConcatTable": 3, "AddTable": 3,
                            "Identity": 3, "Sequential": fx["census"]["Sequential"]}      # (the pool is the reference's own)
    mine = {}
    for m in br.modules():
        if type(m).__module__.startswith("sparse_rcnn_amd") and type(m).__name__ in ("SubmanifoldConvolution", "Convolution",
                                                                                    "AddTable"):
            mine[type(m).__name__] = mine.get(type(m).__name__, 0) + 1
    assert mine == {k: fx["census"][k] for k in mine}
    for line in ("Convolution(32->64 C2/2)", "Convolution(64->128 C2/2)", f"SubmanifoldConvolution({fc}->32 C1)"):
        assert line in fx["repr"] and line in repr(br)


def test_segmentation_head_carries_the_reference_parameters():
    from sparse_rcnn_amd.classhead import SegmentationHead
    fx = _dropin()["segmentation_32"]
    head = SegmentationHead(32, 20)
    kmap, own = head.reference_key_map(), head.named_oracle_params()
    assert set(kmap) == set(fx["keys"])
    for rk, name in kmap.items():
        assert list(own[name].shape) == fx["keys"][rk]
    assert sum(p.numel() for p in head.parameters()) == fx["n_params"] == 32 * 20 + 20
    g = torch.Generator().manual_seed(4)
    sd = {"segmentation_network." + k: torch.randn(shape, generator=g) for k, shape in fx["keys"].items()}
    sd["feature_extractor.unet.module_list.0.channel_changer.weight"] = torch.zeros(1, 64, 32)
    missing, unused = head.load_reference_state_dict(sd)
    assert not missing and not unused
    for rk, name in kmap.items():
        assert torch.equal(own[name], sd["segmentation_network." + rk])
    assert "SubmanifoldConvolution(32->20 C1)" in fx["repr"] and "SubmanifoldConvolution(32->20 C1)" in repr(head)


def test_make_segmentation():
    from sparse_rcnn_amd.synthetic import make_segmentation
    masks = torch.tensor([[1, 0, 0, 1, 0], [1, 1, 0, 0, 0], [0, 1, 0, 1, 1]], dtype=torch.bool)
    labels = torch.tensor([5, 3, 17])
    seg, empty = make_segmentation([labels, torch.zeros(0, dtype=torch.int64)], [masks, torch.zeros((0, 4), dtype=torch.bool)])
    assert seg.dtype == torch.int64 and seg.tolist() == [7, 5, -100, 7, 19]      # overlaps: the lowest-numbered instance
    assert empty.tolist() == [-100] * 4
    assert make_segmentation([labels], [masks], offset=0)[0].tolist() == [5, 3, -100, 5, 17]


def test_scene_step_refuses_without_a_gpu():
    from sparse_rcnn_amd.trainstep import SceneStep
    for wl in ("cfg2", "cfg3", "ref-crop"):
        with pytest.raises(ValueError, match="class_loss=True needs an RPN"):
            SceneStep(wl, device=torch.device("cpu"), class_loss=True)
    for wl in ("cfg2", "cfg5", "ref", "ref-crop"):
        with pytest.raises(ValueError, match="segmentation_loss=True needs a workload with boxes"):
            SceneStep(wl, device=torch.device("cpu"), segmentation_loss=True)


def test_loss_modules_refuse_cpu_and_dtypes():
    from sparse_rcnn_amd import loss as SL
    from sparse_rcnn_amd._lib import ScnError
    with pytest.raises(ScnError):
        SL.CrossEntropyLoss()(torch.zeros(4, 20), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        SL.SegmentationPredictor(sparse=False)
    assert SL.ClassLossSelector(0.1, 0.05, 17).negative_label == 17 and SL.LossFilter(0.1).negative_threshold == 0


# ---- defaults unchanged ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["stand-in", "reference"])
def test_step_model_defaults_unchanged(kind):
    from sparse_rcnn_amd.trainstep import SparseStepModel
    with open(os.path.join(GOLDEN, "stepmodel_params.json")) as f:
        fx = json.load(f)[kind]
    assert (fx["n_tensors"], fx["n_params"]) == {"stand-in": (162, 14050182), "reference": (224, 17820764)}[kind]
    torch.manual_seed(0)
    plain = SparseStepModel(tuple(fx["channels"]), True, False, kind, 64)
    assert [(n, list(p.shape)) for n, p in plain.named_parameters()] == [(n, s) for n, s in fx["params"]]
    assert plain.class_branch is None and plain.segmentation is None
    torch.manual_seed(0)
    full = SparseStepModel(tuple(fx["channels"]), True, False, kind, 64, with_class=True, with_segmentation=True)
    own, other = dict(plain.named_parameters()), dict(full.named_parameters())
    assert set(own) < set(other)
    for n, p in own.items():
        assert torch.equal(p, other[n]), n
    extra = sum(p.numel() for n, p in other.items() if n not in own)
    fc = fx["channels"][3]
    assert extra == {256: 1261426, 80: 1255794}[fc] + 32 * 20 + 20
    assert full.class_level == 3 and full.class_branch.stride == 8
