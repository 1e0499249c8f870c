"""GPU: the class and segmentation losses (csrc/scn_xent.hip behind sparse_rcnn_amd.loss.CrossEntropyLoss / ClassLoss /
ClassLossSelector / ClassPredictor / SegmentationPredictor) against the reference's own outputs (tests/golden/xent_*.npz,
class_loss_*.npz) and the float64 restatement (tests/xent_restate.py); classhead.ClassBranch and SegmentationHead against the
oracle; SceneStep with all four losses, and SceneStep.predict.

Bounds: loss 1e-6 relative, gradient 1e-6 relative L2, probabilities 1e-6 absolute (the RPN- and mask-loss tests' bound;
torch's own fp32 cross_entropy sits within 1.8e-7 / 9.4e-8 of float64); at size FEAT_TOL = 1e-4 of max |oracle| and
FROZEN_L2_F32 = 2e-5 relative L2 (tests/test_gpu_atsize.py)."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import xent_restate as XR                                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(HERE, "golden")
XENT = sorted(glob.glob(os.path.join(GOLDEN, "xent_*.npz")))
CLASS = sorted(glob.glob(os.path.join(GOLDEN, "class_loss_*.npz")))
TOL = 1e-6


def _xid(p):
    return os.path.basename(p)[5:-4]


def _cid(p):
    return os.path.basename(p)[11:-4]


def _run_xent(x, t, w, ignore_index=-100, g=None):
    from sparse_rcnn_amd.loss import CrossEntropyLoss
    crit = CrossEntropyLoss(weight=None if w is None or len(w) == 0 else torch.from_numpy(np.asarray(w)), ignore_index=ignore_index)
    xs = torch.from_numpy(np.ascontiguousarray(x)).to(DEV).requires_grad_()
    loss = crit(xs, torch.from_numpy(np.asarray(t, np.int64)).to(DEV))
    if g is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(g, device=DEV))
    return loss.detach(), xs.grad, crit.n_bad_targets


# ---- 1. the kernel against the fixtures and float64 -------------------------------------------------------------------------
@pytest.mark.parametrize("path", XENT, ids=_xid)
def test_cross_entropy_matches_reference_fixture(path):
    z = np.load(path)
    x, step = XR.fixture_logits(z), int(z["row_step"])
    loss, grad, bad = _run_xent(x, z["targets"], z["weights"])
    loss2, grad2, _ = _run_xent(x, z["targets"], z["weights"])
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    g = grad.cpu().numpy()
    print(f"{_xid(path)}: loss {XR.rel(loss.item(), z['loss']):.2e}  grad {XR.rel_l2(g[::step], z['grad_rows']):.2e}")
    assert XR.rel(loss.item(), z["loss"]) <= TOL
    assert XR.rel_l2(g[::step], z["grad_rows"]) <= TOL
    assert XR.rel(np.sqrt((g.astype(np.float64) ** 2).sum()), z["grad_norm"]) <= TOL
    assert not g[z["targets"] == -100].any() and int(bad.item()) == 0


@pytest.mark.parametrize("weights", [False, True])
def test_cross_entropy_at_segmentation_size(weights):
    n, c = 172_500, 20
    x, t, w = None, None, None
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((n, c)) * 3).astype(np.float32)
    t = rng.integers(0, c, size=n).astype(np.int64)
    t[rng.uniform(size=n) < 0.2] = -100
    w = rng.uniform(0.2, 3.0, c).astype(np.float32) if weights else None
    ref_loss, ref_grad, _ = XR.cross_entropy(x, t, w, g=0.5)
    loss, grad, bad = _run_xent(x, t, w, g=0.5)
    loss2, grad2, _ = _run_xent(x, t, w, g=0.5)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    g = grad.cpu().numpy()
    print(f"172500 x 20 weights={weights}: loss {XR.rel(loss.item(), ref_loss):.2e}  grad {XR.rel_l2(g, ref_grad):.2e}")
    assert XR.rel(loss.item(), ref_loss) <= TOL and XR.rel_l2(g, ref_grad) <= TOL
    assert not g[t == -100].any() and int(bad.item()) == 0


# ---- 2. edge cases ---------------------------------------------------------------------------------------------------------
def test_edge_cases():
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.loss import CrossEntropyLoss
    rng = np.random.default_rng(11)
    # n = 0
    loss, grad, bad = _run_xent(np.zeros((0, 20), np.float32), np.zeros(0, np.int64), None)
    assert loss.item() == 0.0 and grad.shape == (0, 20) and int(bad.item()) == 0
    # every target ignored: loss 0, zero gradient (torch: NaN)
    x = rng.standard_normal((50, 20)).astype(np.float32)
    loss, grad, bad = _run_xent(x, np.full(50, -100), None)
    assert loss.item() == 0.0 and not grad.any().item() and torch.isfinite(grad).all() and int(bad.item()) == 0
    # targets 20 and -5 in a c = 20 problem: dropped and counted, no fault
    t = rng.integers(0, 20, size=50).astype(np.int64)
    t[7], t[31], t[40] = 20, -5, -100
    loss, grad, bad = _run_xent(x, t, None)
    keep = np.ones(50, bool)
    keep[[7, 31, 40]] = False
    ref_loss, ref_grad, ref_bad = XR.cross_entropy(x[keep], t[keep])
    assert int(bad.item()) == 2 == XR.cross_entropy(x, t)[2] and ref_bad == 0
    assert XR.rel(loss.item(), ref_loss) <= TOL and XR.rel_l2(grad.cpu().numpy()[keep], ref_grad) <= TOL
    assert not grad[torch.from_numpy(~keep).to(DEV)].any().item()
    # an ignore_index inside the range drops those rows without counting them
    loss, grad, bad = _run_xent(x, t, None, ignore_index=3)
    ref_loss, ref_grad, ref_bad = XR.cross_entropy(x, t, None, ignore_index=3)
    assert int(bad.item()) == ref_bad == 3 and XR.rel(loss.item(), ref_loss) <= TOL
    assert XR.rel_l2(grad.cpu().numpy(), ref_grad) <= TOL and not grad[torch.from_numpy(t == 3).to(DEV)].any().item()
    # c = 1: loss 0, gradient 0;  c = 256 and a c that is no multiple of 4, each with weights
    loss, grad, _ = _run_xent(rng.standard_normal((9, 1)).astype(np.float32), np.zeros(9, np.int64), None)
    assert loss.item() == 0.0 and not grad.any().item()
    for c in (256, 37, 129, 64, 40, 100, 20, 18, 3):
        x = (rng.standard_normal((333, c)) * 2).astype(np.float32)
        t = rng.integers(0, c, size=333).astype(np.int64)
        t[::5] = -100
        w = rng.uniform(0.2, 3.0, c).astype(np.float32)
        loss, grad, bad = _run_xent(x, t, w)
        ref_loss, ref_grad, _ = XR.cross_entropy(x, t, w)
        assert XR.rel(loss.item(), ref_loss) <= TOL and XR.rel_l2(grad.cpu().numpy(), ref_grad) <= TOL, c
        assert int(bad.item()) == 0
    # refused: c = 257 (the Python module and the C entry point), bf16 logits
    with pytest.raises(L.ScnError):
        CrossEntropyLoss()(torch.zeros((4, 257), device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV))
    x257 = torch.zeros((4, 257), device=DEV)
    t4 = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.zeros((), device=DEV)
    scratch = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    assert L.lib().scn_xent_scratch_bytes(4, 257) == -1 and 0 < L.lib().scn_xent_scratch_bytes(4, 256) <= 1 << 16
    assert L.lib().scn_xent_fwd(L.ptr(x257), 4, 257, L.ptr(t4), None, -100, L.ptr(scratch), L.ptr(out), None,
                                L.stream()) == L.EINVAL
    assert L.lib().scn_softmax_argmax(L.ptr(x257), 4, 257, None, L.ptr(t4), L.stream()) == L.EINVAL
    with pytest.raises(ValueError):
        CrossEntropyLoss()(torch.zeros((4, 20), device=DEV, dtype=torch.bfloat16), t4)
    torch.cuda.synchronize()


# ---- 3. the predictors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", XENT, ids=_xid)
def test_predictors_match_reference_fixture(path):
    from sparse_rcnn_amd.loss import ClassPredictor, SegmentationPredictor
    z = np.load(path)
    x, step, n = XR.fixture_logits(z), int(z["row_step"]), int(z["n"])
    xs = torch.from_numpy(x).to(DEV)
    cls, prob = SegmentationPredictor(sparse=True)(xs)
    assert cls.dtype == torch.int64 and np.array_equal(cls.cpu().numpy(), z["seg_class"])
    assert np.abs(prob.cpu().numpy()[::step].astype(np.float64) - z["prob_rows"]).max() <= TOL
    counts = [n - n // 2, n // 2]
    idx_list, prob_list, raw = ClassPredictor()(xs, (None, counts))
    assert np.array_equal(raw.cpu().numpy(), z["class_indices"]) and [len(i) for i in idx_list] == counts
    assert torch.equal(torch.cat(idx_list), raw) and torch.equal(torch.cat(prob_list), prob)
    if int(z["tie"]):
        assert int(raw[5]) == 3 and int(raw[9]) == 0


def test_predictors_other_widths_and_empty():
    from sparse_rcnn_amd.loss import softmax_argmax, SegmentationPredictor
    rng = np.random.default_rng(5)
    for c in (1, 2, 18, 20, 37, 40, 64, 100, 129, 256):
        x = rng.standard_normal((501, c)).astype(np.float32)
        x[3, c - 1] = x[3, 0] = 9.0                              # first and last column tie
        idx, prob = softmax_argmax(torch.from_numpy(x).to(DEV))
        assert np.array_equal(idx.cpu().numpy(), XR.argmax_first(x)), c
        assert np.abs(prob.cpu().numpy() - XR.softmax(x)).max() <= TOL, c
        idx2, none = softmax_argmax(torch.from_numpy(x).to(DEV), probabilities=False)
        assert none is None and torch.equal(idx, idx2)
    cls, prob = SegmentationPredictor()(torch.zeros((0, 20), device=DEV))
    assert cls.shape == (0,) and cls.dtype == torch.int64 and prob.shape == (0, 20)


# ---- 4. selector + loss against the reference's fixtures -------------------------------------------------------------------
class _Desc:
    def __init__(self, a):
        self.gt_association = a


def _class_inputs(z):
    split = lambda a, counts: list(torch.split(torch.from_numpy(np.asarray(a)).to(DEV), [int(c) for c in counts]))
    labels = split(z["gt_labels"], z["gt_counts"])
    counts = [int(c) for c in z["box_counts"]]
    if int(z["nodesc"]):
        ov = [(None, None, m, a) for m, a in zip(split(z["max_overlap"], z["pred_counts"]), split(z["argmax"], z["pred_counts"]))]
        descs = None
    else:
        ov, descs = None, [_Desc(a) for a in split(z["gt_association"], counts)]
    return labels, counts, ov, descs


@pytest.mark.parametrize("path", CLASS, ids=_cid)
def test_class_loss_matches_reference_fixture(path):
    from sparse_rcnn_amd.loss import ClassLoss, ClassLossSelector
    z = np.load(path)
    labels, counts, ov, descs = _class_inputs(z)
    selector = ClassLossSelector(float(z["positive_threshold"]), float(z["negative_threshold"]), int(z["negative_label"]))
    cw = torch.from_numpy(z["class_weights"]) if len(z["class_weights"]) else None
    outs = []
    for _ in range(2):
        crit = ClassLoss(class_weights=cw)
        scores = torch.from_numpy(z["scores"]).to(DEV).requires_grad_()
        sel_scores, sel_labels = selector(scores, (None, counts), descs, ov, labels)
        loss = crit(sel_scores, sel_labels)
        loss.backward()
        outs.append((loss.detach(), scores.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    full = torch.cat(sel_labels).cpu().numpy()
    assert [len(l) for l in sel_labels] == counts and np.array_equal(full, z["labels_full"])
    valid = [int((l >= 0).sum()) for l in sel_labels]
    assert valid == z["valid_counts"].tolist() and all(v > 0 for v, c in zip(valid, counts) if c)
    assert min(counts) > 0 or _cid(path) == "empty"
    g = scores.grad.cpu().numpy()
    print(f"{_cid(path)}: loss {XR.rel(loss.item(), z['loss']):.2e}  grad {XR.rel_l2(g, z['grad']):.2e}")
    assert XR.rel(loss.item(), z["loss"]) <= TOL and XR.rel_l2(g, z["grad"]) <= TOL
    assert not g[full < 0].any() and int(crit.n_bad_targets.item()) == 0


# ---- 5. no host wait -------------------------------------------------------------------------------------------------------
def test_no_host_wait_from_scores_to_gradient():
    from sparse_rcnn_amd.loss import ClassLoss, ClassLossSelector, ClassPredictor
    z = np.load(os.path.join(GOLDEN, "class_loss_weights.npz"))
    z2 = np.load(os.path.join(GOLDEN, "class_loss_nodesc.npz"))
    one = torch.ones((), device=DEV)
    for zz in (z, z2):
        labels, counts, ov, descs = _class_inputs(zz)
        selector = ClassLossSelector(float(zz["positive_threshold"]), float(zz["negative_threshold"]), int(zz["negative_label"]))
        crit = ClassLoss(class_weights=torch.from_numpy(z["class_weights"]).to(DEV))
        for warm in (True, False):
            scores = torch.from_numpy(zz["scores"]).to(DEV).requires_grad_()
            if not warm:
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")
            try:
                sel_scores, sel_labels = selector(scores, (None, counts), descs, ov, labels)
                loss = crit(sel_scores, sel_labels)
                torch.autograd.backward([loss], [one])
                ClassPredictor()(scores, (None, counts))
            finally:
                torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item() and torch.isfinite(scores.grad).all()


# ---- 8. the step with all four losses --------------------------------------------------------------------------------------
def _torch_xent(scores, targets):
    x = scores.detach().clone().requires_grad_()
    loss = torch.nn.functional.cross_entropy(x, targets, ignore_index=-100)
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("workload,dtype,n_gt", [("cfg3-rpn", "f32", None), ("cfg3-rpn", "bf16", None),
                                                 ("ref-crop-rpn", "f32", 8)])
def test_scenestep_four_losses(workload, dtype, n_gt):
    from sparse_rcnn_amd.trainstep import SceneStep
    st = SceneStep(workload, dtype=dtype, optimizer="adam", rpn_loss=True, mask_loss=True, class_loss=True,
                   segmentation_loss=True, n_gt=n_gt, prefetch=False, lr=1e-4)
    d = st.describe()
    assert "class loss" in d and "segmentation" in d and "mask loss" in d
    st.keep_class_grads = True
    st.step()
    scores, csel, cdescs, sel_labels = st.class_out
    seg_logits, seg_target = st.segmentation_out
    assert scores.dtype == torch.float32 and seg_logits.dtype == torch.float32
    assert scores.grad is not None and seg_logits.grad is not None
    assert st.upstream_grads()[0] is None                       # no seeded gradient on the backbone output
    targets = torch.cat(sel_labels)
    n_gt_total = sum(int(b.shape[0]) for b in st.gt_boxes)
    valid = int((targets >= 0).sum())
    drawn = st.class_selector.last_drawn.cpu()
    share = float((seg_target >= 0).float().mean())
    print(f"[four losses] {workload} {dtype}: class rows {targets.numel()} valid {valid} gt {n_gt_total} drawn {drawn.tolist()} "
          f"segmentation share {share:.3f}")
    assert valid >= n_gt_total and (drawn <= 32).all() and scores.shape == (targets.numel(), 18)
    assert share >= 0.15 and seg_logits.shape == (st.coords.shape[0], 20)
    assert int(((seg_target >= 2) & (seg_target < 20)).sum()) == int((seg_target >= 0).sum())
    for name, x, t, got in (("class", scores, targets, st.class_losses), ("segmentation", seg_logits, seg_target,
                                                                          st.segmentation_losses)):
        ref_loss, ref_grad = _torch_xent(x, t)
        got = float(got.detach().cpu())
        rel = float((x.grad - ref_grad).norm() / ref_grad.norm())
        print(f"[four losses] {name}: loss {got:.6f} vs {float(ref_loss.cpu()):.6f}, gradient rel L2 {rel:.2e}")
        assert abs(got - float(ref_loss.cpu())) <= 1e-5 * abs(float(ref_loss.cpu())), (name, got, float(ref_loss.cpu()))
        assert rel <= 1e-6, (name, rel)
    class_params = {id(p) for p in st.model.class_branch.parameters()}
    saw_class = False
    for p in st.flat.params:
        if p.grad is not None:
            assert torch.isfinite(p.grad).all()
            saw_class |= id(p) in class_params and bool(p.grad.abs().sum() > 0)
    wg = st.model.segmentation.channel_changer.weight.grad
    assert saw_class and wg is not None and torch.isfinite(wg).all() and bool(wg.abs().sum() > 0)
    st.keep_class_grads = False
    series = {"rpn_score": [], "rpn_bbox": [], "mask": [], "class": [], "segmentation": []}

    def record():
        series["rpn_score"].append(float(st.rpn_losses[0].detach().cpu()))
        series["rpn_bbox"].append(float(st.rpn_losses[1].detach().cpu()))
        series["mask"].append(float(st.mask_losses.detach().cpu()))
        series["class"].append(float(st.class_losses.detach().cpu()))
        series["segmentation"].append(float(st.segmentation_losses.detach().cpu()))
    record()
    for _ in range(19):
        st.step()
        record()
    st.finish()
    for name, v in series.items():
        print(f"[four losses] {workload} {dtype} {name}: " + " ".join(f"{x:.4f}" for x in v))
    for name, v in series.items():
        assert np.isfinite(v).all(), name
    for name in ("class", "segmentation"):
        v = series[name]
        assert v[-1] < v[0] and np.mean(v[-5:]) < v[0], (name, v)


# ---- 9. predict ------------------------------------------------------------------------------------------------------------
def test_predict():
    from sparse_rcnn_amd import roi
    from sparse_rcnn_amd.trainstep import SceneStep
    with pytest.raises(ValueError, match="class_loss=True"):
        SceneStep("cfg3-rpn", prefetch=False).predict()
    st = SceneStep("cfg3-rpn", class_loss=True, segmentation_loss=True, prefetch=False)
    out = st.predict()
    st.finish()
    assert {"roi_bbox", "class", "class_propabilities", "mask", "segmentation_class", "segmentation_probabilites"} <= set(out)
    class_scores, logits, (sel, counts, splits) = st.predict_out
    n_kept = [int(b.shape[0]) for b in out["roi_bbox"]]
    assert sum(n_kept) > 0 and n_kept == [int(c) for c in counts] and class_scores.shape == (sum(n_kept), 18)
    ref_idx = torch.argmax(class_scores, 1)
    assert torch.equal(torch.cat(out["class"]), ref_idx)
    assert [tuple(c.shape) for c in out["class"]] == [(n,) for n in n_kept]
    assert [tuple(p.shape) for p in out["class_propabilities"]] == [(n, 18) for n in n_kept]
    assert (torch.cat(out["class_propabilities"]) - torch.softmax(class_scores, 1)).abs().max().item() <= 1e-6
    ref_masks = roi.mask_predict(logits, sel, counts, splits, ref_idx)
    assert len(out["mask"]) == len(ref_masks) == len(n_kept)
    for m, r, n, pts in zip(out["mask"], ref_masks, n_kept, st.splits):
        assert tuple(m.shape) == (n, pts) and torch.equal(m, r)
    assert bool((torch.cat([m.reshape(-1) for m in out["mask"]]) > 0).any())
    n_pts = st.coords.shape[0]
    assert out["segmentation_class"].shape == (n_pts,) and out["segmentation_probabilites"].shape == (n_pts, 20)
    # forward_only keeps its signature and behaviour
    o, lg = st.forward_only()
    st.finish()
    assert lg is not None and lg.shape[1] == 18 and o.features.shape[0] > 0


# ---- 10. the default step holds nothing new ----------------------------------------------------------------------------------
def test_default_step_has_no_class_branch():
    from sparse_rcnn_amd.trainstep import SceneStep
    st = SceneStep("cfg3-rpn", prefetch=False)
    assert st.model.class_branch is None and st.model.segmentation is None
    assert sum(p.numel() for p in st.model.parameters()) == 14050182
    assert not st.class_loss and not st.segmentation_loss and st.class_losses is None and st.segmentation_losses is None
    assert "class loss" not in st.describe() and "segmentation" not in st.describe()


# ---- 6. the class branch against the oracle --------------------------------------------------------------------------------
FEAT_TOL = 1e-4          # tests/test_gpu_atsize.py: forward features, relative to max |oracle|
FROZEN_L2_F32 = 2e-5     # tests/test_gpu_atsize.py: every gradient, relative L2, the device's ReLU decisions frozen into the oracle


class _record_relu_masks:
    def __enter__(self):
        from sparse_rcnn_amd import functional as F
        F.RELU_RECORD = []
        return F.RELU_RECORD

    def __exit__(self, *exc):
        from sparse_rcnn_amd import functional as F
        F.RELU_RECORD = None
        return False


def _rel_scale(a, b):
    return float((a.detach().cpu().double() - b.detach().double()).abs().max() / max(float(b.detach().abs().max()), 1e-30))


def _rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _class_scene(channels, seed=3):
    """A feature map as the stride-8 level of a 512 x 512 x 256 scene: InputLayer on a 64 x 64 x 32 grid, two samples of about
    3 000 active sites; 24 boxes per sample in scene units, two of which catch no site and one pokes out of the scene."""
    import sparse_rcnn_amd as scn
    from sparse_rcnn_amd.synthetic import make_batch
    from sparse_rcnn_amd.tensor import SparseConvNetTensor
    from oracle import scn_oracle as O
    grid = (64, 64, 32)
    coords, _, size, bs, _ = make_batch(2, grid, 3000, dup=1.1, seed=seed)
    feats = torch.randn((coords.shape[0], channels), generator=torch.Generator().manual_seed(seed + 1))
    x = scn.InputLayer(3, size, mode=4)((coords, feats.to(DEV), bs))
    fm = SparseConvNetTensor(features=x.features.detach().clone().requires_grad_(), metadata=x.metadata,
                             spatial_size=x.spatial_size)
    scene = O.OracleScene(coords.numpy())
    rng = np.random.default_rng(seed + 2)
    boxes = []
    for b in range(2):
        sites = scene.coords0[scene.coords0[:, 3] == b][:, :3]
        ctr = sites[rng.integers(0, len(sites), size=24)].astype(np.float64) * 8 + 4
        edge = np.exp(rng.uniform(np.log(16.0), np.log(160.0), size=(24, 3)))
        start = ctr - edge / 2 + rng.uniform(0, 1, size=(24, 3))
        bx = np.stack([start, start + edge], 1)
        occupied = {tuple(s) for s in sites.tolist()}
        empty = [c for c in ((x_, y_, z_) for x_ in range(3, 60, 7) for y_ in range(5, 60, 11) for z_ in range(2, 30, 5))
                 if c not in occupied][:2]
        for i, c in enumerate(empty):                            # inside one coarse cell that holds no site
            bx[5 + 9 * i] = [[(v + 0.2) * 8 for v in c], [(v + 0.7) * 8 for v in c]]
        bx[2, 0, 0], bx[2, 1, 2] = -37.5, 256 + 41.25           # pokes out of the scene on two sides: clipped
        boxes.append(torch.from_numpy(bx.astype(np.float32)))
    return fm, scene, boxes, size


@pytest.mark.parametrize("channels", [256, 80])
def test_class_branch_against_the_oracle(channels):
    import classhead_oracle as CO
    from oracle import scn_oracle as O
    from sparse_rcnn_amd.classhead import ClassBranch
    fm, scene, boxes, size = _class_scene(channels)
    n_sites = [int((scene.coords0[:, 3] == b).sum()) for b in range(2)]
    assert all(2500 <= n <= 3500 for n in n_sites), n_sites
    torch.manual_seed(5)
    br = ClassBranch(channels, 8).to(DEV)
    with _record_relu_masks() as masks:
        scores, (sel, counts, splits) = br(fm, [b.to(DEV) for b in boxes])
    torch.cuda.synchronize()
    assert scores.shape == (48, 18) and scores.dtype == torch.float32 and [int(c) for c in counts] == [24, 24]
    assert len(masks) == 8                                       # 3 units x 2, then the Linear stack's two
    P = {k: p.detach().cpu().clone().requires_grad_() for k, p in br.named_oracle_params().items()}
    X = fm.features.detach().cpu().clone().requires_grad_()
    with torch.no_grad():
        ref, src, box_of, rows = CO.class_branch(scene.coords0, X, P, boxes, size.tolist(), 8)
    # selection bit-equal; the two prepared boxes of each sample are empty, the clipped one is not
    assert np.array_equal(sel.src_row.cpu().numpy().astype(np.int64), src)
    assert np.array_equal(sel.box_of.cpu().numpy().astype(np.int64), box_of)
    assert [int(s) for s in splits] == n_sites
    for b in range(2):
        assert rows[24 * b + 5] == 0 and rows[24 * b + 14] == 0 and rows[24 * b + 2] > 0
    assert int((rows == 0).sum()) >= 4 and int((rows > 0).sum()) >= 40
    e = _rel_scale(scores, ref)
    print(f"[class branch] C={channels}: rows {len(src)}, empty boxes {int((rows == 0).sum())}, scores rel_to_scale {e:.3e}")
    assert e <= FEAT_TOL
    assert torch.isfinite(scores).all()
    empty = torch.from_numpy(rows == 0)
    assert (scores.detach().cpu()[empty] - scores.detach().cpu()[empty][0]).abs().max() == 0   # the bias response
    if channels != 256:
        return
    gs = torch.randn(scores.shape, generator=torch.Generator().manual_seed(9))
    scores.backward(gs.to(DEV))
    torch.cuda.synchronize()
    frozen, _, _, _ = CO.class_branch(scene.coords0, X, P, boxes, size.tolist(), 8, relu=O.FrozenReLU(masks))
    frozen.backward(gs)
    own = br.named_oracle_params()
    assert len(own) == 22
    worst = 0.0
    for k, p in own.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        r = _rel_l2(p.grad, P[k].grad)
        worst = max(worst, r)
        print(f"[class branch] grad {k}: rel L2 {r:.3e}")
        assert r <= FROZEN_L2_F32, (k, r)
    assert torch.isfinite(fm.features.grad).all()
    r = _rel_l2(fm.features.grad, X.grad)
    print(f"[class branch] input gradient rel L2 {r:.3e}; worst parameter {worst:.3e}")
    assert r <= FROZEN_L2_F32


# ---- 7. the segmentation head against the oracle ---------------------------------------------------------------------------
def test_segmentation_head_against_the_oracle():
    import classhead_oracle as CO
    import sparse_rcnn_amd as scn
    from oracle import scn_oracle as O
    from sparse_rcnn_amd.classhead import SegmentationHead
    from sparse_rcnn_amd.synthetic import make_batch
    from sparse_rcnn_amd.tensor import SparseConvNetTensor
    coords, _, size, bs, _ = make_batch(1, (512, 512, 256), 150_000, dup=1.15, seed=1)
    feats = torch.randn((coords.shape[0], 32), generator=torch.Generator().manual_seed(2))
    x = scn.InputLayer(3, size, mode=4)((coords, feats.to(DEV), bs))
    fm = SparseConvNetTensor(features=x.features.detach().clone().requires_grad_(), metadata=x.metadata,
                             spatial_size=x.spatial_size)
    torch.manual_seed(6)
    head = SegmentationHead(32, 20).to(DEV)
    with torch.no_grad():
        head.channel_changer.bias.normal_(0, 0.1)
    out = head(fm)
    assert out.shape == (coords.shape[0], 20) and out.dtype == torch.float32
    gy = torch.randn(out.shape, generator=torch.Generator().manual_seed(3))
    out.backward(gy.to(DEV))
    torch.cuda.synchronize()
    scene = O.OracleScene(coords.numpy())
    assert 140_000 <= scene.n(0) <= 160_000
    X = fm.features.detach().cpu().clone().requires_grad_()
    W = head.channel_changer.weight.detach().cpu().clone().requires_grad_()
    b = head.channel_changer.bias.detach().cpu().clone().requires_grad_()
    ref = CO.segmentation_head(X, scene.prow, W, b)
    ref.backward(gy)
    e = _rel_scale(out, ref)
    rw, rb, rx = (_rel_l2(head.channel_changer.weight.grad, W.grad), _rel_l2(head.channel_changer.bias.grad, b.grad),
                  _rel_l2(fm.features.grad, X.grad))
    print(f"[segmentation head] N={scene.n(0)}: out {e:.3e}  dW {rw:.3e}  db {rb:.3e}  dX {rx:.3e}")
    assert e <= FEAT_TOL and max(rw, rb, rx) <= FROZEN_L2_F32
