"""GPU: the mask loss on the device (sparse_rcnn_amd.loss OverlapCalculator / TrainSelector / MaskLoss, csrc/scn_maskloss.hip)
against the reference's own outputs (tests/golden/mask_loss_*.npz) and the CPU restatement (tests/maskloss_restate.py):
overlaps, the draw (counts, subset, layout, reproducibility, state, uniformity), the loss and its gradient, no host wait, the
packing, and the training step with mask_loss=True."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import maskloss_restate as MS                                  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = sorted(glob.glob(os.path.join(HERE, "golden", "mask_loss_*.npz")))
DEV = "cuda"


def _ids(p):
    return os.path.basename(p)[10:-4]


def _dev(xs, dtype=None):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype) for x in xs]


@pytest.mark.parametrize("path", CASES, ids=_ids)
def test_overlap_matches_reference_fixture(path):
    from sparse_rcnn_amd.loss import OverlapCalculator
    z = np.load(path)
    preds, gts, _, _ = MS.fixture(z)
    out = OverlapCalculator()(_dev(preds), _dev(gts))
    mx = torch.cat([o[2] for o in out]).cpu().numpy()
    am = torch.cat([o[3] for o in out]).cpu().numpy()
    assert np.array_equal(mx.view(np.int32), z["max_overlap"].view(np.int32))
    assert np.array_equal(am, z["argmax"])
    from sparse_rcnn_amd.loss import TrainSelector                 # the one-launch form computes the same overlaps
    ov, _, _ = TrainSelector(0.2).select(_dev(preds), _dev(gts))
    assert np.array_equal(torch.cat([o[2] for o in ov]).cpu().numpy().view(np.int32), z["max_overlap"].view(np.int32))
    assert np.array_equal(torch.cat([o[3] for o in ov]).cpu().numpy(), z["argmax"])


def _draw_sample(g, npos, n_other, G=3):
    """G ground-truth boxes; npos proposals close to one of them (IoU >= 0.2), n_other far from all (IoU 0)."""
    gt = np.array([[[10 + 30 * i, 10, 10], [24 + 30 * i, 26, 22]] for i in range(G)], np.float32)
    near = gt[g.integers(0, G, npos)] + g.uniform(-1, 1, (npos, 2, 3)).astype(np.float32)
    far = np.tile(np.array([[[200, 200, 200], [204, 204, 204]]], np.float32), (n_other, 1, 1))
    far += g.uniform(0, 5, (n_other, 1, 3)).astype(np.float32)
    p = np.concatenate([near, far]).reshape(-1, 2, 3)
    perm = g.permutation(len(p))
    return p[perm].astype(np.float32), gt


def _check_selection(sel, preds, gts, ov, fwd, descs):
    drawn = sel.last_drawn.cpu().numpy()
    for s, (p, g) in enumerate(zip(preds, gts)):
        mx, am = (t.cpu().numpy() for t in ov[s][2:])
        ref_mx, ref_am = MS.overlap(p, g)
        assert np.array_equal(mx.view(np.int32), ref_mx.view(np.int32)) and np.array_equal(am, ref_am)
        npos = int((mx >= np.float32(0.2)).sum())
        nd, cap = min(24, npos), min(24, len(p))
        assert drawn[s] == nd
        d = descs[s]
        ps = d.pred_selection.cpu().numpy()
        assert ps.shape == (cap,) and (ps[nd:] == -1).all()
        picked = ps[:nd]
        assert len(set(picked.tolist())) == nd and (picked >= 0).all() and (mx[picked] >= np.float32(0.2)).all()
        fb = fwd[s].cpu().numpy()
        assert fb.shape == (cap + len(g), 2, 3)
        assert np.array_equal(fb[:nd], p[picked]) and (fb[nd:cap] == 0).all() and np.array_equal(fb[cap:], g)
        a = d.gt_association.cpu().numpy()
        assert np.array_equal(a[:nd], am[picked]) and (a[nd:cap] == -1).all() and np.array_equal(a[cap:], np.arange(len(g)))
        assert np.array_equal(d.gt_selection.cpu().numpy(), np.arange(len(g)))
        assert d.forward_boxes.data_ptr() == fwd[s].data_ptr()


@pytest.mark.parametrize("npos", [0, 1, 7, 23, 24, 25, 60])
def test_draw_counts_and_layout(npos):
    from sparse_rcnn_amd.loss import TrainSelector
    g = np.random.default_rng(npos)
    samples = [_draw_sample(g, npos, 40), _draw_sample(g, 5, 3, G=1), _draw_sample(g, 0, 10, G=2), _draw_sample(g, 30, 200)]
    preds, gts = [s[0] for s in samples], [s[1] for s in samples]
    sel = TrainSelector(0.2, 0, (24, 0, True), seed=11)
    ov, fwd, descs = sel.select(_dev(preds), _dev(gts))
    _check_selection(sel, preds, gts, ov, fwd, descs)
    # the two-step form (OverlapCalculator, then forward) draws the same for the same counter
    from sparse_rcnn_amd.loss import OverlapCalculator
    fwd2, descs2 = sel.draw(OverlapCalculator()(_dev(preds), _dev(gts)), 0)
    for a, b in zip(fwd, fwd2):
        assert torch.equal(a, b)
    for a, b in zip(descs, descs2):
        assert torch.equal(a.gt_association, b.gt_association) and torch.equal(a.pred_selection, b.pred_selection)


def test_padded_slots_select_no_point():
    from sparse_rcnn_amd import roi
    from sparse_rcnn_amd.loss import TrainSelector
    g = np.random.default_rng(3)
    coords = np.concatenate([np.concatenate([g.integers(0, 64, (3000, 3)), np.full((3000, 1), b)], 1) for b in range(2)])
    coords[::50, :3] = 0                                               # points AT the origin, where a padded box sits
    preds = [np.array([[[5, 5, 5], [20, 20, 20]]] * 3, np.float32), np.array([[[40, 40, 40], [44, 44, 44]]] * 30, np.float32)]
    gts = [np.array([[[4, 4, 4], [21, 21, 21]]], np.float32), np.array([[[0, 0, 0], [30, 30, 30]]], np.float32)]
    _, fwd, descs = TrainSelector(0.2).select(_dev(preds), _dev(gts))
    boxes, counts, _ = roi.transform_boxes(list(fwd), (64, 64, 64))
    sel = roi.roi_select(roi._coords_to_device(torch.from_numpy(coords).to(DEV)), boxes)
    rows = np.diff(np.asarray(sel.prefix))
    assoc = torch.cat([d.gt_association for d in descs]).cpu().numpy()
    assert (assoc == -1).sum() == 24 and (rows[assoc == -1] == 0).all() and (rows[assoc >= 0] > 0).all()


def test_draw_reproducible_and_counter_in_state_dict():
    from sparse_rcnn_amd.loss import TrainSelector
    g = np.random.default_rng(5)
    p, gt = _draw_sample(g, 80, 20)
    preds, gts = _dev([p]), _dev([gt])
    sel = TrainSelector(0.2, seed=7)
    first = sel.select(preds, gts)[2][0].pred_selection.clone()
    assert sel.counter == 1
    state = sel.state_dict()
    second = sel.select(preds, gts)[2][0].pred_selection.clone()
    assert sel.counter == 2 and not torch.equal(first, second)
    again = TrainSelector(0.2, seed=99)
    again.load_state_dict(state)
    assert again.seed == 7 and again.counter == 1
    assert torch.equal(again.select(preds, gts)[2][0].pred_selection, second)
    fresh = TrainSelector(0.2, seed=7)
    assert torch.equal(fresh.select(preds, gts)[2][0].pred_selection, first)


def test_draw_uniformity():
    """24 of 100 positives over 400 counters: every positive's frequency within 5 sigma, chi-square within 6 sigma."""
    from sparse_rcnn_amd.loss import OverlapCalculator, TrainSelector
    g = np.random.default_rng(6)
    p, gt = _draw_sample(g, 100, 0, G=1)
    desc = OverlapCalculator()(_dev([p]), _dev([gt]))
    assert int((desc[0][2] >= 0.2).sum()) == 100
    sel = TrainSelector(0.2, seed=2024)
    T = 400
    freq = torch.zeros(100, dtype=torch.float64, device=DEV)
    for c in range(T):
        _, d = sel.draw(desc, c)
        freq.index_add_(0, d[0].pred_selection, torch.ones(24, dtype=torch.float64, device=DEV))
    f = freq.cpu().numpy()
    q = 0.24
    mu, sd = T * q, (T * q * (1 - q)) ** 0.5
    assert f.sum() == T * 24
    assert np.abs(f - mu).max() <= 5 * sd, (f.min(), f.max(), mu, sd)
    chi2 = float(((f - mu) ** 2 / (mu * (1 - q))).sum())                 # ~ chi^2 with 99 dof
    assert 99 - 6 * (2 * 99) ** 0.5 < chi2 < 99 + 6 * (2 * 99) ** 0.5, chi2


def _fixture_loss(z, scores):
    """MaskLoss on the fixture's forward boxes, cropped by the library's crop."""
    from sparse_rcnn_amd import roi
    from sparse_rcnn_amd.loss import MaskLoss, SelectionDescriptor
    _, _, labels, masks = MS.fixture(z)
    counts = [int(c) for c in z["fwd_counts"]]
    fo = np.concatenate([[0], np.cumsum(counts)])
    fwd = [torch.from_numpy(z["fwd_boxes"][fo[s]:fo[s + 1]]).to(DEV) for s in range(len(counts))]
    boxes, _, _ = roi.transform_boxes(fwd, tuple(int(v) for v in z["grid"]))
    sel = roi.roi_select(roi._coords_to_device(torch.from_numpy(z["coords"]).to(DEV)), boxes)
    assoc = torch.from_numpy(z["gt_association"]).to(DEV)
    descs = [SelectionDescriptor(fwd[s], None, None, assoc[fo[s]:fo[s + 1]]) for s in range(len(counts))]
    cw = z["class_weights"]
    crit = MaskLoss(class_weights=torch.from_numpy(cw) if len(cw) else None)
    splits = [int(z["n_pts"])] * len(counts)
    loss = crit(scores, (sel, counts, splits), descs, _dev(labels), _dev(masks))
    return loss, sel


@pytest.mark.parametrize("path", CASES, ids=_ids)
def test_loss_matches_reference_fixture(path):
    z = np.load(path)
    results = []
    for _ in range(2):
        scores = torch.from_numpy(z["scores"]).to(DEV).requires_grad_()
        loss, sel = _fixture_loss(z, scores)
        loss.backward()
        results.append((loss.detach(), scores.grad))
    assert np.array_equal(sel.is_inside().numpy(), MS.fixture_inside(z))
    got, ref = float(results[0][0].cpu()), float(z["loss"])
    assert abs(got - ref) <= 1e-6 * abs(ref), (got, ref)
    g = results[0][1].cpu().numpy().astype(np.float64)
    rel = np.linalg.norm(g - z["grad"]) / np.linalg.norm(z["grad"])
    assert rel <= 1e-6, rel
    for x, y in zip(*results):
        assert torch.equal(x, y)                                       # bitwise identical rerun


def test_empty_boxes_dropped_and_all_empty_gives_zero():
    from sparse_rcnn_amd import roi
    from sparse_rcnn_amd.loss import MaskLoss, SelectionDescriptor
    g = np.random.default_rng(8)
    coords = np.concatenate([g.integers(1, 32, (500, 3)), np.zeros((500, 1), np.int64)], 1)
    labels = [torch.tensor([3, 5], device=DEV)]
    masks = [torch.from_numpy(g.uniform(0, 1, (2, 500)) < 0.5).to(DEV)]
    c32 = roi._coords_to_device(torch.from_numpy(coords).to(DEV))
    for boxes_np, assoc_np in ((np.array([[[0, 0, 0], [0, 0, 0]], [[40, 40, 40], [45, 45, 45]]], np.float32), [-1, 1]),
                               (np.array([[[0, 0, 0], [0, 0, 0]]] * 3, np.float32), [-1, -1, -1])):
        fwd = [torch.from_numpy(boxes_np).to(DEV)]
        boxes, _, _ = roi.transform_boxes(fwd, (64, 64, 64))
        sel = roi.roi_select(c32, boxes)
        assert sel.src_row.shape[0] == 0
        scores = torch.zeros((0, 18), device=DEV, requires_grad=True)
        d = [SelectionDescriptor(fwd[0], None, None, torch.tensor(assoc_np, device=DEV))]
        loss = MaskLoss()(scores, (sel, [len(assoc_np)], [500]), d, labels, masks)
        assert float(loss.cpu()) == 0.0
    # one box with points next to empty ones: the loss is that box's alone
    fwd = [torch.tensor([[[0, 0, 0], [0, 0, 0]], [[4, 4, 4], [20, 20, 20]], [[40, 40, 40], [45, 45, 45]]], device=DEV)]
    boxes, _, _ = roi.transform_boxes(fwd, (64, 64, 64))
    sel = roi.roi_select(c32, boxes)
    m = sel.src_row.shape[0]
    scores = torch.randn((m, 18), device=DEV).requires_grad_()
    assoc = [-1, 0, 1]
    loss = MaskLoss()(scores, (sel, [3], [500]), [SelectionDescriptor(fwd[0], None, None, torch.tensor(assoc, device=DEV))],
                      labels, masks)
    loss.backward()
    ins = sel.is_inside().numpy()
    rl, rg = MS.loss(scores.detach().cpu().numpy(), ins, [3], [500], assoc, np.array([3, 5]), [2], [masks[0].cpu().numpy()])
    assert abs(float(loss.detach().cpu()) - rl) <= 1e-6 * abs(rl)
    assert np.linalg.norm(scores.grad.cpu().numpy() - rg) <= 1e-6 * np.linalg.norm(rg)
    assert (scores.grad.cpu().numpy()[:, [c for c in range(18) if c != 3]] == 0).all()


def test_class_weights_formula():
    z = np.load(os.path.join(HERE, "golden", "mask_loss_weights.npz"))
    assert len(z["class_weights"])
    scores = torch.from_numpy(z["scores"]).to(DEV)
    loss, sel = _fixture_loss(z, scores)
    _, _, labels, masks = MS.fixture(z)
    counts = z["fwd_counts"]
    # sum(w l) / sum(w) against the unweighted mean on the same inputs
    l_w, _ = MS.loss(z["scores"], sel.is_inside().numpy(), counts, [int(z["n_pts"])] * len(counts), z["gt_association"],
                     z["gt_labels"], z["gt_counts"], masks, z["class_weights"])
    l_u, _ = MS.loss(z["scores"], sel.is_inside().numpy(), counts, [int(z["n_pts"])] * len(counts), z["gt_association"],
                     z["gt_labels"], z["gt_counts"], masks, None)
    got = float(loss.cpu())
    assert abs(got - l_w) <= 1e-6 * abs(l_w) and abs(l_w - l_u) > 1e-3


def test_refuses_non_fp32_logits():
    z = np.load(os.path.join(HERE, "golden", "mask_loss_basic.npz"))
    with pytest.raises(ValueError):
        _fixture_loss(z, torch.from_numpy(z["scores"]).to(DEV, torch.bfloat16))


def test_pack_round_trips():
    from sparse_rcnn_amd.loss import pack_gt_masks
    g = np.random.default_rng(9)
    ms = [g.uniform(0, 1, (4, 37)) < 0.4, np.zeros((0, 10), bool), g.uniform(0, 1, (3, 64)) < 0.6, g.uniform(0, 1, (2, 1)) < 0.5]
    ms += [g.uniform(0, 1, (1, 5 + i)) < 0.5 for i in range(35)]      # more samples than one launch's table
    packed = pack_gt_masks(_dev(ms))
    words = packed.words.cpu().numpy().view(np.uint32)
    for s, m in enumerate(ms):
        ref = MS.pack(m)
        got = words[packed.word_offsets[s]:packed.word_offsets[s + 1]].reshape(ref.shape)
        assert np.array_equal(got, ref)
        assert np.array_equal(packed.unpack(s).cpu().numpy(), m)


def test_no_host_wait_on_the_path():
    from sparse_rcnn_amd import roi
    from sparse_rcnn_amd.loss import MaskLoss, TrainSelector, pack_gt_masks
    g = np.random.default_rng(10)
    p, gt = _draw_sample(g, 50, 30)
    preds, gts = _dev([p]), _dev([gt])
    coords = np.concatenate([g.integers(0, 128, (4000, 3)), np.zeros((4000, 1), np.int64)], 1)
    c32 = roi._coords_to_device(torch.from_numpy(coords).to(DEV))
    labels = [torch.tensor([1, 2, 3], device=DEV)]
    packed = pack_gt_masks([torch.from_numpy(g.uniform(0, 1, (3, 4000)) < 0.5).to(DEV)])
    sel_mod, crit = TrainSelector(0.2), MaskLoss()
    one = torch.ones((), device=DEV)
    for warm in (True, False):
        if not warm:
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
        try:
            _, fwd, descs = sel_mod.select(preds, gts)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        boxes, _, _ = roi.transform_boxes(list(fwd), (256, 256, 256))
        sel = roi.roi_select(c32, boxes)                               # (the crop's own selection wait)
        scores = torch.randn((sel.src_row.shape[0], 18), device=DEV).requires_grad_()
        if not warm:
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
        try:
            loss = crit(scores, (sel, [fwd[0].shape[0]], [4000]), descs, labels, packed)
            torch.autograd.backward([loss], [one])
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item() and scores.grad is not None and torch.isfinite(scores.grad).all()


def _torch_restatement(logits, st):
    """The reference's SparseMaskLossSelector + MaskLoss in torch on the step's own logits, selection and ground truth."""
    selection, descs = st.mask_out
    sel, counts, splits = selection
    sc = st._scenes[st._k]
    x = logits.detach().clone().requires_grad_()
    src, prefix = sel.src_row.long().cpu(), sel.prefix
    pt_off = np.concatenate([[0], np.cumsum(splits)])
    assoc = torch.cat([d.gt_association for d in descs]).cpu()
    box_sample = np.repeat(np.arange(len(counts)), counts)
    labels = [l.cpu() for l in sc["gt_label"]]
    per_box = []
    for b in range(sel.n_boxes):
        r0, r1 = prefix[b], prefix[b + 1]
        a = int(assoc[b])
        if a < 0 or r1 == r0:
            continue
        s = int(box_sample[b])
        t = sc["gt_mask_cpu"][s][a][src[r0:r1] - int(pt_off[s])].to(DEV).float()
        per_box.append(torch.nn.functional.binary_cross_entropy_with_logits(x[r0:r1, int(labels[s][a])], t))
    loss = torch.stack(per_box).mean()
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("workload,dtype,n_gt", [("cfg3-rpn", "f32", None), ("cfg3-rpn", "bf16", None),
                                                 ("ref-crop-rpn", "f32", 8)])
def test_scenestep_mask_loss(workload, dtype, n_gt):
    from sparse_rcnn_amd.trainstep import SceneStep
    st = SceneStep(workload, dtype=dtype, optimizer="adam", rpn_loss=True, mask_loss=True, n_gt=n_gt, prefetch=False,
                   lr=1e-4)
    assert "mask loss" in st.describe()
    st.keep_mask_grads = True
    st.step()
    logits = st.logits
    assert logits.dtype == torch.float32 and logits.grad is not None
    ref_loss, ref_grad = _torch_restatement(logits, st)
    got = float(st.mask_losses.detach().cpu())
    assert abs(got - float(ref_loss.cpu())) <= 1e-5 * abs(float(ref_loss.cpu())), (got, float(ref_loss.cpu()))
    rel = float((logits.grad - ref_grad).norm() / ref_grad.norm())
    assert rel <= 1e-6, rel
    mask_params = {id(p) for p in st.model.mask.parameters()}
    saw_mask_grad = False
    for p in st.flat.params:
        if p.grad is not None:
            assert torch.isfinite(p.grad).all()
            saw_mask_grad |= id(p) in mask_params and bool(p.grad.abs().sum() > 0)
    assert saw_mask_grad
    st.keep_mask_grads = False
    drawn = st.mask_selector.last_drawn.cpu()
    assert (drawn <= 24).all()
    # from here on the backbone output gets no seeded synthetic gradient (its FIXED direction drives the features, and with
    # them the mask logits, up within ~10 Adam steps whatever the mask branch learns): the step trains on its two losses
    st._gys[0] = torch.zeros_like(st._gys[0])
    losses = [got]
    for _ in range(19):
        st.step()
        losses.append(float(st.mask_losses.detach().cpu()))
    st.finish()
    print(f"[mask loss] {workload} {dtype}: " + " ".join(f"{v:.4f}" for v in losses))
    assert np.isfinite(losses).all()
    assert losses[-1] < losses[0] and np.mean(losses[-5:]) < losses[0], losses


def test_default_step_keeps_synthetic_mask_gradient():
    from sparse_rcnn_amd.trainstep import SceneStep
    st = SceneStep("cfg3-rpn", prefetch=False)
    st.step()
    st.finish()
    _, gm = st.upstream_grads()
    assert st.mask_losses is None and not st.mask_loss
    assert gm is not None and gm.shape == st.logits.shape and st.logits.shape[0] > 0
