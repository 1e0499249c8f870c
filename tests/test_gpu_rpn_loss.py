"""GPU: the RPN loss on the device (sparse_rcnn_amd.loss, csrc/scn_rpnloss.hip) against the reference's own outputs
(tests/golden/rpn_loss_*.npz) and the CPU restatement (tests/rpnloss_restate.py): anchor targets at both at-size shapes, the
batch-wide draw (exact counts, subset, weights, reproducibility, uniformity), the loss and its gradients, no host wait, and the
training step with rpn_loss=True (gradients at rpn_score / rpn_bbox, loss going down)."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rpnloss_restate as RS                                   # noqa: E402

pytestmark = pytest.mark.gpu
CASES = sorted(glob.glob(os.path.join(HERE, "golden", "rpn_loss_*.npz")))
DEV = "cuda"


def _ids(p):
    return os.path.basename(p)[9:-4]


def _gt_list(z):
    o = z["gt_offsets"]
    return [torch.from_numpy(z["gt_boxes"][o[i]:o[i + 1]]).to(DEV) for i in range(len(o) - 1)]


def _check_targets(got, ref):
    ov, am, tg = (t.cpu().numpy() for t in got)
    assert np.array_equal(ov.view(np.int32), ref[0].view(np.int32))
    assert np.array_equal(am, ref[1])
    assert RS.ulp_diff(tg, ref[2]).max() <= 2


@pytest.mark.parametrize("path", CASES, ids=_ids)
def test_targets_match_reference_fixture(path):
    from sparse_rcnn_amd.loss import rpn_target_calculator
    z = np.load(path)
    calc = rpn_target_calculator(torch.from_numpy(z["inside_anchors"]).to(DEV))
    _check_targets(calc(_gt_list(z)), (z["max_overlaps"], z["argmax"], z["bbox_targets"]))


def _random_boxes(g, n, scene, lo=8.0, hi=96.0):
    scene = np.asarray(scene, np.float64)
    ctr = g.uniform(0, 1, (n, 3)) * scene
    edge = np.exp(g.uniform(np.log(lo), np.log(hi), (n, 3)))
    start = ctr - edge / 2
    return np.stack([start, start + edge], 1).astype(np.float32)


def _stand_in_calculator():
    from sparse_rcnn_amd.rpn import DenseRpn
    rpn = DenseRpn(256, stride=8).to(DEV)
    return rpn.target_calculator((64, 64, 32)), (512, 512, 256)          # cfg3-rpn: 395 136 inside anchors


def _ref_crop_calculator():
    from sparse_rcnn_amd.rpn import MultiLevelRpn, REF_ANCHOR_LEVELS_VOXELS
    rpn = MultiLevelRpn([(64, 4, 128, REF_ANCHOR_LEVELS_VOXELS[0]), (80, 8, 256, REF_ANCHOR_LEVELS_VOXELS[1])],
                        num_dilations=5).to(DEV)
    return rpn.target_calculator((128, 128, 64)), (128, 128, 64)


@pytest.mark.parametrize("shape", ["cfg3-rpn", "ref-crop-rpn"])
def test_targets_at_size(shape):
    calc, scene = _stand_in_calculator() if shape == "cfg3-rpn" else _ref_crop_calculator()
    g = np.random.default_rng(11)
    counts = [64] if shape == "cfg3-rpn" else [256] * 9 + [0, 1, 1500]   # 0, 1 and three LDS chunks of boxes
    boxes = [_random_boxes(g, c, scene, 4.0, 64.0) for c in counts]
    got = calc([torch.from_numpy(b).to(DEV) for b in boxes])
    if shape == "cfg3-rpn":
        assert calc.anchors.shape[0] == 395136
    else:
        assert calc.anchors.shape[0] == 36240
    offs = np.cumsum([0] + counts)
    ref = RS.targets(calc.anchors.cpu().numpy(), np.concatenate(boxes) if sum(counts) else np.zeros((0, 2, 3), np.float32),
                     offs)
    _check_targets(got, ref)
    ov = got[0].cpu().numpy()
    assert (ov >= 0.35).sum() > 0 and (ov < 0.15).sum() > 0


def _selector(seed=0):
    from sparse_rcnn_amd.loss import BatchwiseBboxTargetSelector
    return BatchwiseBboxTargetSelector(0.35, 0.15, max_weight=1 / 8, seed=seed)


def _check_draw(ov_np, out, counts):
    labels, sw, bw = (t.cpu().numpy() for t in out)
    pos, neg = ov_np >= np.float32(0.35), ov_np < np.float32(0.15)
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    assert counts.cpu().tolist() == [n_pos, n_neg]
    larger, smaller = (pos, neg) if n_pos > n_neg else (neg, pos)
    chosen = sw > 0
    assert (chosen & ~(larger | smaller)).sum() == 0                   # only members of the two sets
    assert (chosen & smaller).sum() == smaller.sum() if min(n_pos, n_neg) else chosen.sum() == 0
    drawn = chosen & larger
    assert drawn.sum() == min(n_pos, n_neg)                           # exact count, a subset of the larger set
    ref = RS.weights_for(ov_np, drawn)
    for got, r in zip((labels, sw, bw), ref):
        assert np.array_equal(got, r)
    return drawn


def _sampler_inputs():
    out = {}
    for p in CASES:
        out[_ids(p)] = np.load(p)["max_overlaps"]
    g = np.random.default_rng(3)
    out["random_pos_lt_neg"] = g.uniform(0, 0.5, (3, 5000)).astype(np.float32)
    out["random_pos_gt_neg"] = g.uniform(0.1, 1.0, (2, 7000)).astype(np.float32)
    out["equal"] = np.array([[0.5] * 300 + [0.0] * 300 + [0.2] * 50], np.float32)
    out["no_positives"] = np.zeros((2, 100), np.float32)
    out["nothing"] = np.full((1, 64), 0.2, np.float32)
    return out


@pytest.mark.parametrize("name", sorted(_sampler_inputs()))
def test_sampler_cases(name):
    ov_np = _sampler_inputs()[name]
    ov = torch.from_numpy(ov_np).to(DEV)
    sel = _selector(seed=9)
    d1 = _check_draw(ov_np, sel.draw(ov, 4), sel.last_counts)
    a = [t.clone() for t in sel.draw(ov, 4)]
    b = sel.draw(ov, 4)
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                      # same seed + counter: bit-identical
    d2 = _check_draw(ov_np, sel.draw(ov, 5), sel.last_counts)
    pos, neg = (ov_np >= np.float32(0.35)).sum(), (ov_np < np.float32(0.15)).sum()
    if 0 < min(pos, neg) and max(pos, neg) >= 50 and min(pos, neg) < max(pos, neg):
        assert not np.array_equal(d1, d2)                             # another counter: another draw


def test_selector_counter_advances_and_restores():
    ov = torch.from_numpy(_sampler_inputs()["random_pos_lt_neg"]).to(DEV)
    sel = _selector(seed=1)
    first = [t.clone() for t in sel(ov)]
    state = sel.state_dict()
    second = [t.clone() for t in sel(ov)]
    assert not torch.equal(first[1], second[1])
    again = _selector(seed=123)
    again.load_state_dict(state)
    for x, y in zip(again(ov), second):
        assert torch.equal(x, y)


def test_sampler_uniformity():
    """100 of 1000 negatives drawn (100 positives) over 400 counters: every negative's frequency inside a binomial bound."""
    ov_np = np.array([[0.9] * 100 + [0.0] * 1000], np.float32)
    ov = torch.from_numpy(ov_np).to(DEV)
    sel = _selector(seed=2024)
    freq = torch.zeros(1100, dtype=torch.float64, device=DEV)
    T = 400
    for c in range(T):
        _, sw, _ = sel.draw(ov, c)
        freq += (sw[0] > 0).double()
    f = freq.cpu().numpy()
    assert (f[:100] == T).all()
    neg = f[100:]
    p = 0.1
    mu, sd = T * p, (T * p * (1 - p)) ** 0.5
    assert neg.sum() == T * 100
    assert np.abs(neg - mu).max() <= 5 * sd, (neg.min(), neg.max(), mu, sd)     # 5 sigma per index: p ~ 6e-7 each
    chi2 = float(((neg - mu) ** 2 / (mu * (1 - p))).sum())                      # ~ chi^2 with 999 dof
    assert 999 - 6 * (2 * 999) ** 0.5 < chi2 < 999 + 6 * (2 * 999) ** 0.5, chi2


def _loss_on(z):
    from sparse_rcnn_amd.loss import RpnLoss
    t = {k: torch.from_numpy(z[k]).to(DEV) for k in ("rpn_score", "rpn_bbox", "labels", "score_weight", "bbox_targets",
                                                   "bbox_weights")}
    score = t["rpn_score"].clone().requires_grad_()
    bbox = t["rpn_bbox"].clone().requires_grad_()
    prep = (None, None, t["bbox_targets"], t["labels"], t["score_weight"], t["bbox_weights"])
    sl, bl = RpnLoss(_selector()).loss(prep, score, bbox)
    (sl + bl).backward()
    return sl, bl, score.grad, bbox.grad


@pytest.mark.parametrize("path", CASES, ids=_ids)
def test_loss_matches_reference_fixture(path):
    z = np.load(path)
    sl, bl, gs, gb = _loss_on(z)
    for got, ref in ((sl, z["score_loss"]), (bl, z["bbox_loss"])):
        got, ref = float(got.detach().cpu()), float(ref)
        assert abs(got - ref) <= 1e-6 * abs(ref) or got == ref == 0.0, (got, ref)
    assert RS.close_grad(gs.cpu().numpy(), z["grad_score"])
    assert RS.close_grad(gb.cpu().numpy(), z["grad_bbox"])
    again = _loss_on(z)
    for x, y in zip((sl, bl, gs, gb), again):
        assert torch.equal(x, y)                                     # bitwise identical rerun


def test_loss_at_size_deterministic_and_matches_restatement():
    from sparse_rcnn_amd.loss import RpnLoss
    calc, scene = _ref_crop_calculator()
    g = np.random.default_rng(5)
    boxes = [torch.from_numpy(_random_boxes(g, 256, scene, 4.0, 64.0)).to(DEV) for _ in range(12)]
    crit = RpnLoss(_selector(seed=3))
    N = calc.anchors.shape[0]
    gen = torch.Generator(device=DEV).manual_seed(0)
    score0 = torch.randn((12, N), device=DEV, generator=gen) * 2
    bbox0 = torch.randn((12, N, 2, 3), device=DEV, generator=gen) * 0.3
    results = []
    for _ in range(2):
        crit.bbox_target_selector.counter = 0
        score, bbox = score0.clone().requires_grad_(), bbox0.clone().requires_grad_()
        sl, bl = crit(boxes, calc, score, bbox)
        (sl + bl).backward()
        results.append((sl, bl, score.grad, bbox.grad))
    for x, y in zip(*results):
        assert torch.equal(x, y)
    _, _, tg, lab, sw, bw = (t.cpu().numpy() if t is not None else None for t in crit.last_prepared)
    rs = RS.loss(score0.cpu().numpy(), bbox0.cpu().numpy(), lab, sw, tg, bw)
    sl, bl, gs, gb = results[0]
    assert abs(float(sl.detach().cpu()) - rs[0]) <= 1e-6 * abs(rs[0]) and abs(float(bl.detach().cpu()) - rs[1]) <= 1e-6 * abs(rs[1])
    assert RS.close_grad(gs.cpu().numpy(), rs[2]) and RS.close_grad(gb.cpu().numpy(), rs[3])


def test_no_host_wait_on_the_path():
    from sparse_rcnn_amd.loss import RpnLoss
    calc, scene = _stand_in_calculator()
    g = np.random.default_rng(1)
    boxes = [torch.from_numpy(_random_boxes(g, 64, scene)).to(DEV)]
    crit = RpnLoss(_selector())
    N = calc.anchors.shape[0]
    score = torch.zeros((1, N), device=DEV, requires_grad=True)
    bbox = torch.zeros((1, N, 2, 3), device=DEV, requires_grad=True)
    one = torch.ones((), device=DEV)
    sl, bl = crit(boxes, calc, score, bbox)                          # warm-up: workspaces, scratch
    torch.autograd.backward([sl, bl], [one, one])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        prep = crit.prepare(boxes, calc)
        sl, bl = crit.loss(prep, score, bbox)
        torch.autograd.backward([sl, bl], [one, one])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(sl).item() and torch.isfinite(bl).item()


# the mean RPN loss (score + bbox) over the last 5 of 30 Adam steps relative to step 1's stays below 0.85 (calibrated on an
# MI355X: 0.730 cfg3-rpn f32, 0.732 cfg3-rpn bf16, 0.727 ref-crop-rpn f32, 0.727 ref-crop-rpn bf16)
LOSS_DROP = 0.85


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("workload", ["cfg3-rpn", "ref-crop-rpn"])
def test_scenestep_rpn_loss(workload, dtype):
    from sparse_rcnn_amd.trainstep import SceneStep
    # Adam at 3e-5: at the reference's 4e-4 the FIXED synthetic gradient on the backbone output drives the cfg3-rpn backbone
    # features (and with them the RPN's loss) up within 10 steps, whatever the RPN learns
    st = SceneStep(workload, dtype=dtype, optimizer="adam", rpn_loss=True, prefetch=False, lr=3e-5)
    assert "RPN loss" in st.describe()
    st.keep_rpn_grads = True
    st.step()                                                        # step 1: forward + backward + Adam
    rpn_bbox, rpn_score = st.rpn_out[0], st.rpn_out[1]
    _, _, tg, lab, sw, bw = (t.cpu().numpy() for t in st.rpn_criterion.last_prepared)
    rs = RS.loss(rpn_score.detach().cpu().numpy(), rpn_bbox.detach().cpu().numpy(), lab, sw, tg, bw)
    assert RS.close_grad(rpn_score.grad.cpu().numpy(), rs[2])
    assert RS.close_grad(rpn_bbox.grad.cpu().numpy(), rs[3])
    sl, bl = (float(t.detach().cpu()) for t in st.rpn_losses)
    assert abs(sl - rs[0]) <= 1e-5 * abs(rs[0]) and abs(bl - rs[1]) <= 1e-5 * abs(rs[1])
    st.keep_rpn_grads = False
    losses = [sl + bl]
    for _ in range(29):
        st.step()
        losses.append(float(sum(t.detach() for t in st.rpn_losses).cpu()))
    st.finish()
    ratio = float(np.mean(losses[-5:])) / losses[0]
    print(f"[rpn loss] {workload} {dtype}: step 1 {losses[0]:.5g}, last 5 mean {np.mean(losses[-5:]):.5g}, ratio {ratio:.4f}")
    assert np.isfinite(losses).all()
    assert ratio < LOSS_DROP, losses
