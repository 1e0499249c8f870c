"""Device time of the mask-loss kernels (scn_mask_overlap_draw, scn_mask_loss, scn_mask_loss_bwd) at the cfg3-rpn and
ref-crop-rpn (n_gt = 8) sizes, against a torch restatement of the reference's code path run on the GPU with the same inputs
(OverlapCalculator per sample; TrainSelector with its torch.where / len host waits and a numpy draw; SparseMaskLossSelector's
split by is_inside.sum(1).tolist() and per-box masks; MaskLoss's per-box BCE, isnan filter and mean through autograd), and
SceneStep ms/step with and without mask_loss.

    python tools/mask_loss_bench.py [--out profiles/mask_loss.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=50, warm=5):
    """mean ms per call, events around `reps` back-to-back calls (the host waits inside fn are part of it)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


# ---- the reference's torch formulation (restated from ndsis/modules/model.py and ndsis/modules/loss.py) ---------------------
def torch_overlap(pred, gt):
    if len(gt) == 0:
        return pred.new_zeros(len(pred)), pred.new_zeros(len(pred), dtype=torch.long)
    sa, ea, sb, eb = pred[:, None, 0], pred[:, None, 1], gt[None, :, 0], gt[None, :, 1]
    inter = (torch.min(ea, eb) - torch.max(sa, sb)).clamp(min=0).prod(-1)
    ov = inter / ((ea - sa).prod(-1) + (eb - sb).prod(-1) - inter)
    return ov.max(1)


def torch_select(pred, gt, mx, am, num_pos=24):
    pos, = torch.where(mx >= 0.2)
    pick = torch.tensor(np.random.choice(len(pos), min(len(pos), num_pos), replace=False), dtype=torch.long).to(pos.device)
    use = pos[pick]
    g = torch.arange(len(gt), device=gt.device)
    return torch.cat((pred[use], gt[g])), torch.cat((am[use], g))


def torch_loss(scores, is_inside, counts, assoc_list, labels, masks):
    split = torch.split(scores, is_inside.sum(1).tolist())             # (host wait, as the reference's .tolist())
    ins = torch.split(is_inside, counts)
    l, b = [], 0
    for s, a_s in enumerate(assoc_list):
        lab, gm = labels[s][a_s], masks[s][a_s]
        for j in range(len(a_s)):
            t = gm[j][ins[s][j][pt_off[s]:pt_off[s + 1]]].float()
            l.append(F.binary_cross_entropy_with_logits(split[b][:, lab[j]], t))
            b += 1
    ls = torch.stack(l)
    ls = ls[~torch.isnan(ls)]
    return ls.mean() if len(ls) else scores.new_zeros(())


pt_off = None


def case(label, n_samples, grid, target, n_props, n_gt, out):
    global pt_off
    from sparse_rcnn_amd import roi
    from sparse_rcnn_amd.loss import MaskLoss, TrainSelector, pack_gt_masks
    from sparse_rcnn_amd.synthetic import make_batch, make_boxes, make_instances
    dev = torch.device("cuda")
    coords, _, _, _, splits = make_batch(n_samples, grid, target, dup=1.15, seed=1)
    gts = [b[:n_gt] for b in make_boxes(coords, n_gt, seed=3)]
    g = np.random.default_rng(4)
    preds = []
    for gb in gts:
        src = gb.numpy()[g.integers(0, len(gb), n_props)].astype(np.float64)
        size = src[:, 1] - src[:, 0]
        start = src[:, 0] + g.uniform(-0.3, 0.3, (n_props, 3)) * size
        stop = np.maximum(src[:, 1] + g.uniform(-0.3, 0.3, (n_props, 3)) * size, start + 1)
        preds.append(torch.from_numpy(np.stack([start, stop], 1).astype(np.float32)).to(dev))
    gts = [b.to(dev) for b in gts]
    labels_cpu, masks_cpu = make_instances(coords, [b.cpu() for b in gts])
    labels = [l.to(dev) for l in labels_cpu]
    masks = [m.to(dev) for m in masks_cpu]
    packed = pack_gt_masks(masks)
    c32 = roi._coords_to_device(coords.to(dev))
    ts, crit = TrainSelector(0.2, seed=1), MaskLoss()
    _, fwd, descs = ts.select(preds, gts)
    boxes, counts, _ = roi.transform_boxes(list(fwd), grid)
    sel = roi.roi_select(c32, boxes)
    m = sel.src_row.shape[0]
    scores = torch.randn((m, 18), device=dev).requires_grad_()
    one = torch.ones((), device=dev)
    npos = sum(int((o[2] >= 0.2).sum()) for o in ts.select(preds, gts)[0])

    def draw():
        ts.select(preds, gts)

    def lossf():
        return crit(scores, (sel, counts, splits), descs, labels, packed)

    def fb():
        torch.autograd.backward([lossf()], [one])

    t_draw, t_loss, t_fb = timed(draw), timed(lossf), timed(fb)

    def dev_all():
        _, f2, d2 = ts.select(preds, gts)
        torch.autograd.backward([crit(scores, (sel, counts, splits), d2, labels, packed)], [one])
    t_all = timed(dev_all)
    # torch: the same inputs; the crop's dense is_inside of the same forward boxes
    pt_off = np.concatenate([[0], np.cumsum(splits)])
    is_inside = sel.is_inside_u8().bool()
    np.random.seed(0)

    def tdraw():
        return [torch_select(p, gb, *torch_overlap(p, gb)) for p, gb in zip(preds, gts)]

    assoc = [d.gt_association[d.gt_association >= 0] for d in descs]
    keep = torch.cat([d.gt_association >= 0 for d in descs])
    ins_kept = is_inside[keep]
    rows = ins_kept.sum(1)
    kept_counts = [int((d.gt_association >= 0).sum()) for d in descs]
    sc_rows = torch.cat([torch.arange(a, b, device=dev) for a, b, k in
                         zip(sel.prefix[:-1], sel.prefix[1:], keep.tolist()) if k]) if m else torch.zeros(0, dtype=torch.long)
    scores_kept = scores.detach()[sc_rows].requires_grad_()

    def tfb():
        torch_loss(scores_kept, ins_kept, kept_counts, assoc, labels, masks).backward()

    r_draw, r_fb = timed(tdraw, reps=10, warm=2), timed(tfb, reps=5, warm=1)
    line = (f"{label}: {n_samples} sample(s), {n_props} proposals and {n_gt} ground truths each ({npos} positives), "
            f"{sel.n_boxes} forward boxes, {m} cropped rows\n"
            f"  device  overlap+draw {t_draw:.4f}  loss {t_loss:.4f}  loss+backward {t_fb:.4f}  all (draw + loss + backward, incl. "
            f"host launch cost) {t_all:.4f} ms\n"
            f"  torch   overlap+draw {r_draw:.4f}  loss+backward {r_fb:.4f}  all {r_draw + r_fb:.4f} ms (host waits included)\n")
    print(line, end="", flush=True)
    out.append(line)


def step_case(workload, dtype, out, n_gt=None, steps=10):
    from sparse_rcnn_amd.trainstep import SceneStep
    res = []
    for ml in (False, True):
        st = SceneStep(workload, dtype=dtype, optimizer="adam", rpn_loss=True, mask_loss=ml, n_gt=n_gt, prefetch=False, lr=3e-5)
        for _ in range(3):
            st.step()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            st.step()
        st.finish()
        b.record()
        torch.cuda.synchronize()
        res.append((a.elapsed_time(b) / steps, st.n_roi_rows))
        del st
    line = (f"SceneStep {workload} {dtype} adam 3e-5 rpn_loss{'' if n_gt is None else f' n_gt={n_gt}'}: {res[0][0]:.3f} ms/step "
            f"with the synthetic mask gradient (24 best-scored or all proposals, {res[0][1]} cropped points), {res[1][0]:.3f} "
            f"ms/step with mask_loss=True ({res[1][1]} cropped points) ({steps} steps)\n")
    print(line, end="", flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_loss.txt"))
    args = ap.parse_args()
    torch.manual_seed(0)
    out = [f"# mask loss on the device vs a torch restatement of the reference's path ({torch.cuda.get_device_name()}); "
           "ms per call, CUDA events around back-to-back calls\n"]
    case("cfg3-rpn", 1, (512, 512, 256), 150_000, 64, 64, out)
    case("ref-crop-rpn n_gt=8", 12, (128, 128, 64), 12_500, 256, 8, out)
    step_case("cfg3-rpn", "f32", out)
    step_case("ref-crop-rpn", "bf16", out, n_gt=8)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.writelines(out)


if __name__ == "__main__":
    main()
