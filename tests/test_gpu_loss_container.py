"""GPU: the loss container -- scn_loss_combine / scn_loss_combine_bwd, sparse_rcnn_amd.loss.Loss and SceneStep(multitask_loss=,
loss_weights=) -- against the fixtures of the reference's own `Loss` (tests/golden/loss_container_*.npz) and the float64
restatement (tests/loss_container_restate.py).  Every bound is the derived one: 16 units of 2^-24 times the quantity's scale."""
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_container_restate as RS                            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CASES = sorted(glob.glob(os.path.join(HERE, "golden", "loss_container_*.npz")))
ID = lambda p: os.path.basename(p)[len("loss_container_"):-4]     # noqa: E731
NEEDED = dict(mask_positive_threshold=0.2, class_positive_threshold=0.1, class_negative_threshold=0, class_negative_label=-100)


def _scalars(values, present=None):
    return [torch.tensor(float(v), dtype=torch.float32, device=DEV) if (present is None or present[i]) else None
            for i, v in enumerate(values)]


def _within(got, ref, scale, what, units=RS.UNITS):
    err, b = abs(float(got) - float(ref)), float(RS.bound(scale, units))
    print(f"{what}: got {float(got):.9g} ref {float(ref):.9g} |err| {err:.3e} bound {b:.3e}")
    assert err <= b, what


# ---- 1. the kernel against every fixture ------------------------------------------------------------------------------------
def _run_kernel(z, scale, weight_grads=None, running=None):
    from sparse_rcnn_amd import loss as RL
    root = torch.full((5,), -3.0, device=DEV)
    rec = RL.loss_combine(_scalars(z["terms"], z["present"]), _scalars(z["params"]), scale, root_grad=root,
                          weight_grads=weight_grads, running=running)
    return rec, root


@pytest.mark.parametrize("path", CASES, ids=ID)
def test_kernel_matches_fixture_and_restatement(path):
    z = np.load(path)
    present = z["present"]
    scale = 1.0 / 3.0
    r = RS.combine(z["terms"], present, z["params"], scale)
    SENTINEL = 7.0
    wg = [torch.tensor(0.0 if r["weight_used"][j] else SENTINEL, device=DEV) for j in range(5)]
    running = torch.zeros(9, dtype=torch.float64, device=DEV)
    rec, root = _run_kernel(z, scale, wg, running)
    rec_h, root_h = rec.cpu().numpy(), root.cpu().numpy()
    first = np.array([float(g) for g in wg], np.float32)
    # the record: totals within the bound of the restatement (so is the fixture: tests/test_loss_container_cpu.py), the terms exact
    _within(rec_h[0], r["total"], r["S_total"], "_total_")
    _within(rec_h[1], r["total_multitask"], r["S_multitask"], "_total_multitask_")
    _within(rec_h[0], z["total"], 2 * r["S_total"], "_total_ against the fixture")
    _within(rec_h[1], z["total_multitask"], 2 * r["S_multitask"], "_total_multitask_ against the fixture")
    assert np.array_equal(rec_h[2:7], np.where(present, z["terms"], np.float32(0)))
    assert rec_h[7] == 0
    for i in range(5):
        if present[i]:
            _within(root_h[i], r["term_grad"][i], r["S_term_grad"][i], f"root_grad[{i}]")
        else:
            assert root_h[i] == 0
    for j in range(5):
        if r["weight_used"][j]:
            _within(first[j], r["weight_grad"][j], r["S_weight_grad"][j], f"weight_grad[{j}]")
        else:
            assert first[j] == SENTINEL                          # an absent term leaves its weight's slot alone
    # a second call accumulates: exactly twice the first (x + x is exact), within the bound of twice the restatement
    rec2, root2 = _run_kernel(z, scale, wg, running)
    second = np.array([float(g) for g in wg], np.float32)
    for j in range(5):
        if r["weight_used"][j]:
            assert second[j] == np.float32(2) * first[j]
            _within(second[j], 2 * r["weight_grad"][j], 2 * r["S_weight_grad"][j], f"weight_grad[{j}] after two calls")
        else:
            assert second[j] == SENTINEL
    assert torch.equal(rec, rec2) and torch.equal(root, root2)                           # bitwise identical rerun
    run = running.cpu().numpy()
    assert run[8] == 2 and np.array_equal(run[:8], 2 * rec_h.astype(np.float64))
    # `scale` is applied: a power of two scales exactly
    _, root1 = _run_kernel(z, 1.0)
    wg_half = [torch.zeros((), device=DEV) for _ in range(5)]
    wg_one = [torch.zeros((), device=DEV) for _ in range(5)]
    rec_half, root_half = _run_kernel(z, 0.5, wg_half)
    _run_kernel(z, 1.0, wg_one)
    assert torch.equal(root_half, root1 * 0.5)
    assert torch.equal(torch.stack(wg_half), torch.stack(wg_one) * 0.5)
    assert torch.equal(rec_half, rec)                                                    # the record does not depend on it
    # all weights 1: the plain fp32 sum in the reference's order, and nothing added for the weights
    if ID(path).startswith("unit"):
        assert rec_h[0].view(np.int32) == RS.plain_sum_f32(z["terms"], present).view(np.int32)
        assert rec_h[1].view(np.int32) == rec_h[0].view(np.int32)
        assert rec_h[0].view(np.int32) == z["total"].view(np.int32)


def test_kernel_backward_form_and_argument_checks():
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd import loss as RL
    z = np.load(os.path.join(HERE, "golden", "loss_container_no_class_mask.npz"))
    terms, ws = _scalars(z["terms"], z["present"]), _scalars(z["params"])
    g = torch.tensor(0.75, device=DEV)
    buf = torch.full((10,), 5.0, device=DEV)
    L.check(L.lib().scn_loss_combine_bwd(g.data_ptr(), RL._pointer_table(terms), RL._pointer_table(ws), buf.data_ptr(),
                                         buf.data_ptr() + 20, L.stream()))
    r = RS.combine(z["terms"], z["present"], z["params"], 0.75)
    h = buf.cpu().numpy()
    for i in range(5):
        if z["present"][i]:
            _within(h[i], r["term_grad"][i], r["S_term_grad"][i], f"term_grad[{i}]")
        else:
            assert h[i] == 0
        if r["weight_used"][i]:
            _within(h[5 + i], r["weight_grad"][i], r["S_weight_grad"][i], f"weight_grad[{i}]")
        else:
            assert h[5 + i] == 0
    # the calls validate: a missing log-weight, a missing record, a scale that is not finite, a misaligned pointer
    lib = L.lib()
    rec = torch.zeros(8, device=DEV)
    tp, wp = RL._pointer_table(terms), RL._pointer_table(ws)
    bad_w = RL._pointer_table(ws[:4] + [None])
    assert lib.scn_loss_combine(tp, bad_w, 1.0, rec.data_ptr(), None, None, None, L.stream()) == L.EINVAL
    assert lib.scn_loss_combine(tp, wp, 1.0, None, None, None, None, L.stream()) == L.EINVAL
    assert lib.scn_loss_combine(tp, wp, float("inf"), rec.data_ptr(), None, None, None, L.stream()) == L.EINVAL
    assert lib.scn_loss_combine(tp, wp, 1.0, rec.data_ptr() + 2, None, None, None, L.stream()) == L.EINVAL
    assert lib.scn_loss_combine_bwd(None, tp, wp, buf.data_ptr(), None, L.stream()) == L.EINVAL
    assert lib.scn_loss_combine_bwd(g.data_ptr(), tp, bad_w, buf.data_ptr(), None, L.stream()) == L.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(rec, torch.zeros(8, device=DEV))                                  # a refused call wrote nothing
    with pytest.raises(ValueError):
        RL.loss_combine(terms[:4], ws)
    with pytest.raises(ValueError):
        RL.loss_combine([torch.zeros(1, device=DEV)] + terms[1:], ws)
    with pytest.raises(ValueError):
        RL.loss_combine(terms, ws, root_grad=torch.zeros(4, device=DEV))


# ---- 2. Loss through autograd on fixture terms ----------------------------------------------------------------------------
def _loss_for(z, **kw):
    from sparse_rcnn_amd.loss import Loss, WEIGHT_NAMES
    calc = dict(zip(("calc_bbox", "calc_class", "calc_mask", "calc_segmentation"), (bool(c) for c in z["calc"])))
    cw = dict(zip(WEIGHT_NAMES, (float(w) for w in z["ctor_weights"])))
    loss = Loss(batchwise_subsample=True, sparse=True, multitask_loss=bool(z["multitask"]), **cw, **calc, **NEEDED, **kw).to(DEV)
    with torch.no_grad():
        for n, v in zip(WEIGHT_NAMES, z["params"]):
            getattr(loss, n).copy_(torch.tensor(float(v)))
    return loss


@pytest.mark.parametrize("path", CASES, ids=ID)
def test_loss_autograd_on_fixture_terms(path):
    from sparse_rcnn_amd.loss import WEIGHT_NAMES
    z = np.load(path)
    present = z["present"]
    loss = _loss_for(z)
    assert all(p.requires_grad == bool(z["multitask"]) for p in loss.log_weights())
    terms = [t.requires_grad_() if t is not None else None for t in _scalars(z["terms"], present)]
    combined, rec = loss.combine(terms)
    assert combined.dim() == 0 and combined.is_cuda and combined.grad_fn is not None
    upstream = 0.5                                               # (loss / batches_per_step).backward()
    (combined * upstream).backward()
    r = RS.combine(z["terms"], present, z["params"], upstream)
    _within(combined.detach().cpu(), r["total_multitask"], r["S_multitask"], "combined")
    for i in range(5):
        if present[i]:
            _within(terms[i].grad.cpu(), r["term_grad"][i], r["S_term_grad"][i], f"term grad {i}")
            _within(terms[i].grad.cpu() / upstream, z["term_grad"][i], 2 * r["S_term_grad"][i] / upstream, f"term grad {i} (fixture)")
    for j, n in enumerate(WEIGHT_NAMES):
        p = getattr(loss, n)
        if bool(z["weight_has_grad"][j]):
            _within(p.grad.cpu(), r["weight_grad"][j], r["S_weight_grad"][j], n)
            _within(p.grad.cpu() / upstream, z["weight_grad"][j], 2 * r["S_weight_grad"][j] / upstream, n + " (fixture)")
        else:
            assert p.grad is None, n                             # the weight of an absent term, or multitask_loss off
    if not bool(z["multitask"]) and ID(path) == "all_fixed":     # fixed non-unit weights scale the term gradients
        got = np.array([float(t.grad) for t in terms]) / upstream
        want = np.exp(-z["params"].astype(np.float64))[[1, 0, 2, 3, 4]]
        assert np.abs(want - 1).min() > 0.4 and np.allclose(got, want, rtol=1e-6)
    # the mapping: the reference's keys in its order, floats after one copy, read-only
    assert list(rec) == list(z["subloss_keys"])
    assert rec["_total_multitask_"] == float(combined.detach().cpu())
    assert [rec[k] for k in list(rec)[2:]] == [float(v) for v in z["terms"][present]]
    assert not rec.isnan and rec.tensor.shape == (8,) and rec.tensor.is_cuda
    with pytest.raises(TypeError):
        rec["_total_"] = 0.0
    with pytest.raises(KeyError):
        rec["nan_terms"]
    assert loss.get_weights().keys() == dict(zip(z["get_weights_keys"], z["get_weights_values"])).keys()
    for k, v in zip(z["get_weights_keys"], z["get_weights_values"]):
        assert abs(loss.get_weights()[k] - float(v)) <= 8 * RS.EPS * float(v)       # exp on either side within 2 ulp of 2^-23
    means = loss.running_means()
    assert means["steps"] == 1 and means["_total_"] == rec["_total_"] and means["nan_terms"] == 0
    loss.reset_running()
    assert loss.running_means() == {}


# ---- 3. / 4. Loss on real criteria, without a host wait -------------------------------------------------------------------------
def _real_inputs():
    from sparse_rcnn_amd.loss import rpn_target_calculator
    z = np.load(os.path.join(HERE, "golden", "rpn_loss_two_levels.npz"))
    x = np.load(os.path.join(HERE, "golden", "xent_300x18_u_s1.npz"))
    o = z["gt_offsets"]
    gt = [torch.from_numpy(z["gt_boxes"][o[i]:o[i + 1]]).to(DEV) for i in range(len(o) - 1)]
    calc = rpn_target_calculator(torch.from_numpy(z["inside_anchors"]).to(DEV))
    leaves = [torch.from_numpy(a).to(DEV).requires_grad_() for a in (z["rpn_score"], z["rpn_bbox"], x["logits"])]
    targets = torch.from_numpy(x["targets"]).to(DEV)
    return gt, calc, leaves, targets


def _container(seed):
    from sparse_rcnn_amd.loss import Loss
    return Loss(batchwise_subsample=True, sparse=True, seed=seed, positive_overlap=0.35, negative_overlap=0.15, max_weight=1 / 8,
                calc_bbox=True, calc_class=False, calc_mask=False, calc_segmentation=True, **NEEDED).to(DEV)


def _by_hand(seed):
    from sparse_rcnn_amd.loss import BatchwiseBboxTargetSelector, CrossEntropyLoss, RpnLoss
    gt, calc, (score, bbox, logits), targets = _real_inputs()
    sl, bl = RpnLoss(BatchwiseBboxTargetSelector(0.35, 0.15, max_weight=1 / 8, seed=seed), 2.)(gt, calc, score, bbox)
    seg = CrossEntropyLoss(None, ignore_index=-100)(logits, targets)
    total = (sl + bl) + seg                                      # the reference's order; 0 + sl is sl
    total.backward()
    return total.detach(), (sl.detach(), bl.detach(), seg.detach()), (score.grad, bbox.grad, logits.grad)


def test_loss_on_real_criteria_is_bit_equal_to_the_criteria_by_hand():
    total, parts, grads = _by_hand(seed=3)
    gt, calc, (score, bbox, logits), targets = _real_inputs()
    loss = _container(seed=3)
    combined, rec = loss(dict(gt_bbox=gt, gt_segmentation=targets),
                         dict(rpn_score=score, rpn_bbox=bbox, rpn_target_calculator=calc, spn_segmentation=logits, is_training=True))
    combined.backward()
    assert torch.equal(combined.detach(), total)
    for got, ref in zip((score.grad, bbox.grad, logits.grad), grads):
        assert torch.equal(got, ref)
    assert all(p.grad is None for p in loss.log_weights())
    assert list(rec) == ["_total_", "_total_multitask_", "rpn_score", "rpn_bbox", "segmentation"]
    assert [rec[k] for k in rec] == [float(total)] * 2 + [float(p) for p in parts]


def test_no_host_wait_in_forward_and_backward():
    total, parts, _ = _by_hand(seed=3)
    gt, calc, (score, bbox, logits), targets = _real_inputs()
    loss = _container(seed=3)
    batch = dict(gt_bbox=gt, gt_segmentation=targets)
    outputs = dict(rpn_score=score, rpn_bbox=bbox, rpn_target_calculator=calc, spn_segmentation=logits, is_training=True)
    one = torch.ones((), device=DEV)
    combined, _ = loss(batch, outputs)                           # warm-up: workspaces, scratch, the running record
    torch.autograd.backward([combined], [one])
    loss.rpn_loss.bbox_target_selector.counter = 0               # the draw of the call by hand
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        combined, rec = loss(batch, outputs)
        torch.autograd.backward([combined], [one])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    fixture = np.load(os.path.join(HERE, "golden", "loss_container_no_class_mask.npz"))
    assert list(rec) == list(fixture["subloss_keys"])            # the reference's keys and order for RPN + segmentation
    assert rec["_total_"] == float(total) and rec["segmentation"] == float(parts[2])
    assert loss.running_means()["steps"] == 2


# ---- 5. NaN handling -------------------------------------------------------------------------------------------------------------
def test_nan_term_is_counted_and_waits_for_nothing():
    z = np.load(os.path.join(HERE, "golden", "loss_container_all_multitask.npz"))
    loss = _loss_for(z)
    vals = z["terms"].copy()
    terms = [t.requires_grad_() for t in _scalars(vals)]
    loss.combine(terms)[0].backward()                            # warm-up
    vals[3] = np.nan
    terms = [t.requires_grad_() for t in _scalars(vals)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        combined, rec = loss.combine(terms)
        combined.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert math.isnan(rec["_total_"]) and math.isnan(rec["_total_multitask_"]) and math.isnan(rec["mask"])
    assert rec.isnan and float(rec.tensor[7]) == 1.0
    assert not math.isnan(rec["rpn_score"]) and math.isfinite(float(terms[0].grad))
    clean, rec0 = loss.combine([t.detach() for t in _scalars(z["terms"])])
    assert not rec0.isnan and math.isfinite(rec0["_total_"])


# ---- 6. - 8. SceneStep ---------------------------------------------------------------------------------------------------------
FOUR = dict(rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True)


def _step_terms(st):
    t = [st.rpn_losses[0], st.rpn_losses[1], st.class_losses, st.mask_losses, st.segmentation_losses]
    return np.array([float(x.detach().cpu()) for x in t], np.float64)


def test_scenestep_with_learned_weights():
    from sparse_rcnn_amd.trainstep import SceneStep
    kw = dict(optimizer="adam", lr=3e-5, prefetch=False, **FOUR)
    st = SceneStep("cfg3-rpn", multitask_loss=True, loss_weights=dict(segmentation=0.125, rpn_bbox=0.5), **kw)
    assert "loss container" in st.describe() and "scn_loss_combine" in st.describe()
    ws = st.combiner.log_weights()
    lo, hi = st.flat.flat.data_ptr(), st.flat.flat.data_ptr() + 4 * st.flat.flat.numel()
    assert all(lo <= p.data_ptr() < hi for p in ws) and all(any(p is q for q in st.flat.params) for p in ws)   # in the flat buffer
    w0 = np.array([float(p.detach().cpu()) for p in ws], np.float32)
    assert np.array_equal(w0, (-torch.log(torch.tensor([1, 0.5, 1, 1, 0.125], dtype=torch.float32))).numpy())
    assert st.loss_weights() == pytest.approx({"rpn_score": 1.0, "rpn_bbox": 0.5, "class": 1.0, "mask": 1.0, "segment": 0.125})
    st.keep_rpn_grads = True
    st.forward_backward(0)
    terms = _step_terms(st)
    r = RS.combine(terms, [True] * 5, w0)
    grads = [p.grad for p in ws]
    assert all(g is not None and g.data_ptr() == v.data_ptr() for g, v in zip(grads, st._weight_grad_views))
    g_host = np.array([float(g.cpu()) for g in grads])
    for j in range(5):
        _within(g_host[j], r["weight_grad"][j], r["S_weight_grad"][j], f"log-weight gradient {j}")
    rec = st.loss_record
    assert list(rec) == ["_total_", "_total_multitask_", "rpn_score", "rpn_bbox", "class", "mask", "segmentation"]
    assert [rec[k] for k in list(rec)[2:]] == [float(np.float32(t)) for t in terms]
    _within(rec["_total_multitask_"], r["total_multitask"], r["S_multitask"], "record total")
    score_grad = st.rpn_out[1].grad.detach().clone()
    # the update: every weight moves against the sign of its gradient
    st.adam.lr = st.lr
    st.flat.adam_step_single_rank(st.adam)
    w1 = np.array([float(p.detach().cpu()) for p in ws], np.float32)
    assert (g_host != 0).all() and np.array_equal(np.sign(w1.astype(np.float64) - w0), -np.sign(g_host))
    # the gradient at rpn_score against a step with unit weights and the same seeds: exp(-w[rpn_bbox]) times it
    unit = SceneStep("cfg3-rpn", **kw)
    assert unit.combiner is None
    unit.keep_rpn_grads = True
    unit.forward_backward(0)
    assert torch.equal(unit.rpn_out[1].detach(), st.rpn_out[1].detach())
    ref = unit.rpn_out[1].grad.double() * math.exp(-float(w0[1]))
    err = (score_grad.double() - ref).abs()
    ulp = torch.maximum(ref.abs(), torch.tensor(2.0 ** -126, device=DEV, dtype=torch.float64)) * 2.0 ** -23
    worst = float((err / ulp).max())
    print(f"rpn_score gradient against exp(-w) x the unit-weight step's: worst {worst:.3f} ulp")
    assert worst <= 4
    # loss.Loss on the tensors this micro-batch produced: the class and mask criteria behind the reference's keys give the
    # step's own values, in training mode (the selectors' descriptors) and over all boxes (overlaps + LossFilter)
    from sparse_rcnn_amd.loss import Loss
    sc = unit._scenes[0]
    class_scores, csel, cdescs, _ = unit.class_out
    selection, descs = unit.mask_out
    crit = Loss(batchwise_subsample=True, sparse=True, calc_bbox=False, calc_class=True, calc_mask=True, calc_segmentation=False,
                **NEEDED).to(DEV)
    batch = dict(gt_bbox=sc["gt_dev"], gt_label=sc["gt_label"], gt_mask=sc["gt_mask"])
    cls = dict(mpn_class=class_scores.detach(), mpn_class_coord_selection=csel, mpn_class_box_selection=cdescs)
    msk = dict(mpn_mask=unit.logits.detach(), mpn_mask_coord_selection=selection, mpn_mask_box_selection=descs)
    combined, rec = crit(batch, dict(is_training=True, **cls, **msk))
    assert list(rec) == ["_total_", "_total_multitask_", "class", "mask"]
    want = (float(unit.class_losses.detach().cpu()), float(unit.mask_losses.detach().cpu()))
    assert (rec["class"], rec["mask"]) == want
    assert rec["_total_"] == float(np.float32(want[0]) + np.float32(want[1])) == float(combined)
    cls["mpn_class_box_selection"] = msk["mpn_mask_box_selection"] = None
    _, rec_c = crit(batch, dict(is_training=False, roi_bbox=[d.forward_boxes for d in cdescs], **cls))
    _, rec_m = crit(batch, dict(is_training=False, roi_bbox=[d.forward_boxes for d in descs], **msk))
    assert list(rec_c) == ["_total_", "_total_multitask_", "class"] and list(rec_m) == ["_total_", "_total_multitask_", "mask"]
    assert (rec_c["class"], rec_m["mask"]) == want
    st.finish()
    unit.finish()


def test_scenestep_with_fixed_weights_has_no_parameters_to_learn():
    from sparse_rcnn_amd.trainstep import SceneStep
    st = SceneStep("cfg3-rpn", optimizer="adam", lr=3e-5, prefetch=False, rpn_loss=True, loss_weights=dict(rpn_bbox=0.5))
    assert st.combiner is not None and not st.multitask_loss and "fixed weights" in st.describe()
    ws = st.combiner.log_weights()
    assert not any(p.requires_grad for p in ws) and not any(any(p is q for q in st.flat.params) for p in ws)
    assert sum(p.numel() for p in st.flat.params) == 14050182            # the default step's parameters (test_gpu_class_loss.py)
    st.step()
    st.finish()
    assert list(st.loss_record) == ["_total_", "_total_multitask_", "rpn_score", "rpn_bbox"]
    assert st.loss_weights() == pytest.approx({"rpn_score": 1.0, "rpn_bbox": 0.5})
    root = st._root_grad.cpu().numpy()
    # rpn_score is scaled by the rpn_bbox weight, rpn_bbox by the rpn_class weight (the reference's crossing); the rest is absent
    _within(root[0], 0.5, 0.5, "root gradient of rpn_score")
    assert root[1] == 1.0 and (root[2:] == 0).all()
    assert all(p.grad is None for p in ws)


@pytest.mark.parametrize("packed", [False, True], ids=["fast-path", "packed"])
def test_scenestep_weights_of_losses_that_are_off_get_no_gradient(packed, monkeypatch):
    """multitask_loss with the RPN loss alone: only its two log-weights get a gradient and move; the three others keep
    `grad is None` and their values.  packed: the update reads the packed flat buffer (what several ranks, buckets and
    count-weighting use), where the parameters without a gradient are zero-filled next to the kernel-filled views."""
    from sparse_rcnn_amd.trainstep import SceneStep
    if packed:
        monkeypatch.setenv("SCN_STEP_PACKED", "1")
    st = SceneStep("cfg3-rpn", optimizer="adam", lr=3e-5, prefetch=False, rpn_loss=True, multitask_loss=True,
                   loss_weights=dict(rpn_bbox=0.5))
    ws = st.combiner.log_weights()
    w0 = np.array([float(p.detach().cpu()) for p in ws], np.float32)
    st.step()
    st.finish()
    assert all(p.grad is not None for p in ws[:2]) and all(p.grad is None for p in ws[2:])
    terms = np.array([float(t.detach().cpu()) for t in st.rpn_losses] + [0, 0, 0], np.float64)
    r = RS.combine(terms, [True, True, False, False, False], w0)
    g_host = np.array([float(p.grad.cpu()) for p in ws[:2]])
    for j in range(2):
        _within(g_host[j], r["weight_grad"][j], r["S_weight_grad"][j], f"log-weight gradient {j}")
    if packed:
        index = {id(p): i for i, p in enumerate(st.flat.params)}
        packed_g = [float(st.flat.mean_grad_views()[index[id(p)]].cpu()) for p in ws]
        assert packed_g[:2] == list(g_host) and packed_g[2:] == [0.0, 0.0, 0.0]
    w1 = np.array([float(p.detach().cpu()) for p in ws], np.float32)
    assert np.array_equal(w1[2:], w0[2:])
    assert (g_host != 0).all() and np.array_equal(np.sign(w1[:2].astype(np.float64) - w0[:2]), -np.sign(g_host))


def test_scenestep_accumulates_the_weight_gradients_over_micro_batches():
    from sparse_rcnn_amd.trainstep import SceneStep
    st = SceneStep("cfg3-rpn", optimizer="adam", lr=3e-5, prefetch=False, multitask_loss=True, batches_per_step=2,
                   loss_weights=dict(segmentation=0.125, rpn_bbox=0.5), **FOUR)
    ws = st.combiner.log_weights()
    w0 = np.array([float(p.detach().cpu()) for p in ws], np.float32)
    with st.flat.accumulate():
        st.forward_backward(0, zero=True)
    r0 = RS.combine(_step_terms(st), [True] * 5, w0, 0.5)
    st.forward_backward(1, zero=False)
    r1 = RS.combine(_step_terms(st), [True] * 5, w0, 0.5)
    for j, p in enumerate(ws):
        _within(p.grad.cpu(), r0["weight_grad"][j] + r1["weight_grad"][j], r0["S_weight_grad"][j] + r1["S_weight_grad"][j],
                f"accumulated log-weight gradient {j}", units=2 * RS.UNITS)
    assert st.combiner.running_means()["steps"] == 2
    st.finish()


def test_scenestep_defaults_build_no_container():
    from sparse_rcnn_amd import loss as RL
    from sparse_rcnn_amd.trainstep import SceneStep
    before = RL.combine_launches
    st = SceneStep("cfg3-rpn", prefetch=False)
    # the text of a step built without the new arguments, of one built with their defaults spelled out, and of one whose
    # weights are all 1: the same, before any step has run
    explicit = SceneStep("cfg3-rpn", prefetch=False, multitask_loss=False, loss_weights=None)
    assert explicit.combiner is None and st.describe() == explicit.describe()
    del explicit
    assert st.combiner is None and st.loss_record is None and not hasattr(st.model, "loss_combiner")
    assert sum(p.numel() for p in st.model.parameters()) == 14050182          # (tests/test_gpu_class_loss.py: the default step)
    st.step()
    st.finish()
    assert RL.combine_launches == before                         # the container's kernel is not launched
    d = st.describe()
    assert "loss container" not in d and "scn_loss_combine" not in d
    assert st.loss_weights() == {}
