"""Device time of the RPN loss kernels (scn_rpn_targets, scn_rpn_sample_batchwise, scn_rpn_loss + backward scale) at the
cfg3-rpn and ref-crop-rpn sizes, against the reference's torch formulation of the same steps run on the GPU with the same
inputs (select_bbox over 2^18-anchor chunks + bbox_transform; the batch-wide selector with its nonzero / len host waits and a
numpy draw; BCE-with-logits + smooth L1 through autograd), and SceneStep ms/step with and without rpn_loss.

    python tools/rpn_loss_bench.py [--out profiles/rpn_loss.txt]
"""
import argparse
import os
import sys
import time

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


# ---- the reference's torch formulation (restated from ndsis/utils/bbox.py and ndsis/modules/loss.py) ----------------------
def torch_targets(anchors, gt_list, chunk=2 ** 18):
    a_pos, a_size = anchors[:, 0], anchors[:, 1]
    half = a_size / 2
    a_start, a_end = a_pos - half, a_pos + half
    a_area = a_size.prod(-1)
    ovs, ams, rois = [], [], []
    for g in gt_list:
        if len(g):
            g_start, g_end = g[:, 0], g[:, 1]
            g_area = (g_end - g_start).prod(-1)
            parts = []
            for s in range(0, anchors.shape[0], chunk):
                lo = torch.max(a_start[s:s + chunk, None], g_start[None])
                hi = torch.min(a_end[s:s + chunk, None], g_end[None])
                inter = (hi - lo).clamp(min=0).prod(-1)
                parts.append(inter / (a_area[s:s + chunk, None] + g_area[None] - inter))
            ov, am = torch.cat(parts, 0).max(1)
            roi = g[am]
        else:
            ov = torch.zeros_like(anchors[:, 0, 0])
            am = torch.full_like(ov, -1, dtype=torch.long)
            roi = torch.zeros_like(anchors)
        ovs.append(ov)
        ams.append(am)
        rois.append(roi)
    roi = torch.stack(rois)
    size = roi[..., 1, :] - roi[..., 0, :]
    pos = roi[..., 0, :] + 0.5 * size
    d_pos = (pos - a_pos) / (a_size + 1e-14)
    d_size = torch.log(size / (a_size + 1e-14) + 1e-14)
    return torch.stack(ovs), torch.stack(ams), torch.stack([d_pos, d_size], -2)


def torch_select(ov):
    pos, neg = ov >= 0.35, ov < 0.15
    pi, ni = torch.nonzero(pos), torch.nonzero(neg)
    pc, nc = len(pi), len(ni)
    sub = np.random.choice(max(pc, nc), size=min(pc, nc), replace=False)
    if pc > nc:
        sw, idx = neg.float(), pi[sub]
    else:
        sw, idx = pos.float(), ni[sub]
    sw[idx.unbind(-1)] = 1
    sw /= max(1, 2 * min(pc, nc))
    lab = pos.float()
    return lab, sw, lab / lab.sum().clamp(min=8.0)


def torch_loss(score, bbox, lab, sw, tg, bw, sigma=2.0):
    sl = F.binary_cross_entropy_with_logits(score, lab, sw, reduction="sum")
    s2 = sigma ** 2
    d = bbox - tg
    a = d.abs()
    m = (a < 1 / s2).detach().float()
    bl = (bw[..., None, None] * (d * d * (s2 / 2) * m + (a - 0.5 / s2) * (1 - m))).sum()
    return sl, bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpn_loss.txt"))
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.loss import BatchwiseBboxTargetSelector, RpnLoss
    from sparse_rcnn_amd.rpn import DenseRpn, MultiLevelRpn, REF_ANCHOR_LEVELS_VOXELS
    from sparse_rcnn_amd.synthetic import make_batch, make_boxes
    from sparse_rcnn_amd.trainstep import SceneStep, WORKLOADS
    dev = torch.device("cuda")
    lines = [f"# RPN loss on the device vs the reference's torch formulation ({torch.cuda.get_device_name(0)}); "
             "ms per call, CUDA events around back-to-back calls"]
    for wl in ("cfg3-rpn", "ref-crop-rpn"):
        ch, grid, target, nb, _, ns = WORKLOADS[wl]
        coords, _, size, bs, _ = make_batch(ns, grid, target, dup=1.15, seed=1)
        boxes = [b.to(dev) for b in make_boxes(coords, nb, seed=3)]
        if wl == "cfg3-rpn":
            calc = DenseRpn(ch[-1], stride=8).to(dev).target_calculator(tuple(g // 8 for g in grid))
        else:
            rpn = MultiLevelRpn([(ch[2], 4, 128, REF_ANCHOR_LEVELS_VOXELS[0]), (ch[3], 8, 256, REF_ANCHOR_LEVELS_VOXELS[1])])
            calc = rpn.to(dev).target_calculator(grid)
        N, B = calc.anchors.shape[0], len(boxes)
        sel = BatchwiseBboxTargetSelector()
        crit = RpnLoss(sel)
        gt, offs = calc._concat(boxes)
        ov, am, tg = calc.from_concatenated(gt, offs)
        lab, sw, bw = sel(ov)
        gen = torch.Generator(device=dev).manual_seed(0)
        score = (torch.randn((B, N), device=dev, generator=gen) * 2).requires_grad_()
        bbox = (torch.randn((B, N, 2, 3), device=dev, generator=gen) * 0.3).requires_grad_()
        one = torch.ones((), device=dev)
        prep = (ov, am, tg, lab, sw, bw)
        t_tg = timed(lambda: calc.from_concatenated(gt, offs))
        t_sel = timed(lambda: sel(ov))
        t_loss = timed(lambda: crit.loss(prep, score, bbox))

        def fb():
            sl, bl = crit.loss(prep, score, bbox)
            torch.autograd.backward([sl, bl], [one, one])
        t_lb = timed(fb)
        t_all = timed(lambda: (lambda p: torch.autograd.backward(list(crit.loss(p, score, bbox)), [one, one]))(
            crit.prepare(boxes, calc)))
        np.random.seed(0)
        r_tg = timed(lambda: torch_targets(calc.anchors, boxes), reps=10, warm=2)
        r_sel = timed(lambda: torch_select(ov), reps=10, warm=2)

        def rfb():
            sl, bl = torch_loss(score, bbox, lab, sw, tg, bw)
            (sl + bl).backward()
        r_lb = timed(rfb, reps=10, warm=2)

        def rall():
            o, _, t = torch_targets(calc.anchors, boxes)
            l_, s_, b_ = torch_select(o)
            sl, bl = torch_loss(score, bbox, l_, s_, t, b_)
            (sl + bl).backward()
        r_all = timed(rall, reps=10, warm=2)
        n_pos, n_neg = sel.last_counts.tolist()
        lines.append(f"{wl}: {B} sample(s) x {N} inside anchors, {sum(len(b) for b in boxes)} boxes ({B * N * nb / 1e6:.1f} M IoUs), "
                     f"{n_pos} pos / {n_neg} neg")
        lines.append(f"  device  targets {t_tg:.4f}  sample {t_sel:.4f}  loss {t_loss:.4f}  loss+backward {t_lb:.4f}  "
                     f"all (prepare + loss + backward, incl. host launch cost) {t_all:.4f} ms")
        lines.append(f"  torch   targets {r_tg:.4f}  sample {r_sel:.4f}  loss+backward {r_lb:.4f}  all {r_all:.4f} ms "
                     "(the selector's host waits included)")
        print("\n".join(lines[-3:]), flush=True)
        del calc, crit, score, bbox
    for wl in ("cfg3-rpn", "ref-crop-rpn"):
        for dtype in ("f32", "bf16"):
            res = []
            for flag in (False, True):
                st = SceneStep(wl, dtype=dtype, optimizer="adam", rpn_loss=flag, lr=3e-5)
                for _ in range(3):
                    st.step()
                st.finish()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    st.step()
                st.finish()
                torch.cuda.synchronize()
                res.append((time.perf_counter() - t0) * 1e3 / args.steps)
                res.append(st.n_roi_rows)
                del st
                torch.cuda.empty_cache()
            lines.append(f"SceneStep {wl} {dtype} adam 3e-5: {res[0]:.3f} ms/step with the synthetic RPN gradient ({res[1]} cropped "
                         f"points), {res[2]:.3f} ms/step with rpn_loss=True ({res[3]} cropped points) ({args.steps} steps)")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
