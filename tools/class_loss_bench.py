"""Device time of the cross-entropy kernels (scn_xent_fwd, scn_xent_bwd behind loss.CrossEntropyLoss) at the segmentation sizes
(172 500 and 600 000 points, 20 classes) and the class sizes (96 and 480 rows, 18 classes) against
torch.nn.functional.cross_entropy forward + backward on the same device tensors, the two alternating; the class path end to
end (draw, branch forward, loss, backward) at the cfg3-rpn and ref-crop-rpn sizes; SceneStep ms/step with and without the
class and segmentation losses.

    python tools/class_loss_bench.py [--out profiles/class_loss.txt] [--no-steps]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 200


def timed(fn, reps=REPS, warm=10):
    """mean ms per call, events around `reps` back-to-back calls."""
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


def xent_case(n, c, out, rounds=3):
    from sparse_rcnn_amd.loss import CrossEntropyLoss
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(n)
    x = (torch.randn((n, c), generator=g) * 3).to(dev).requires_grad_()
    t = torch.randint(0, c, (n,), generator=g)
    t[torch.rand(n, generator=g) < 0.2] = -100
    t = t.to(dev)
    one = torch.ones((), device=dev)
    crit = CrossEntropyLoss()

    def ours():
        x.grad = None
        torch.autograd.backward([crit(x, t)], [one])

    def theirs():
        x.grad = None
        torch.autograd.backward([F.cross_entropy(x, t, ignore_index=-100)], [one])

    a, b = [], []
    for _ in range(rounds):                                      # alternating
        a.append(timed(ours))
        b.append(timed(theirs))
    out.append(f"cross entropy fwd+bwd n={n} c={c}: device {min(a):.4f} ms (runs {' '.join(f'{v:.4f}' for v in a)}), "
               f"torch {min(b):.4f} ms (runs {' '.join(f'{v:.4f}' for v in b)}), torch / device {min(b) / min(a):.2f}x; "
               f"{REPS} repetitions per run, {2 if n <= 2048 else 3} launches (rows{'' if n <= 2048 else ', finish'}, backward), "
               f"logits read twice and the gradient written once = {3 * n * c * 4 / 1e6:.1f} MB")


def class_path_case(label, workload, n_gt, out):
    """draw + branch forward + loss + backward on the step's own feature level and proposals."""
    from sparse_rcnn_amd.trainstep import SceneStep
    st = SceneStep(workload, optimizer="adam", rpn_loss=True, class_loss=True, n_gt=n_gt, prefetch=False, lr=3e-5)
    st.step()
    st.finish()
    m, sc = st.model, st._scenes[0]
    level = m.backbone.unet.interims[m.class_level]
    from sparse_rcnn_amd.tensor import SparseConvNetTensor
    fm = SparseConvNetTensor(features=level.features.detach().float().requires_grad_(), metadata=level.metadata,
                             spatial_size=level.spatial_size)
    proposals = [b.detach() for b in st.rpn_out[4]]
    one = torch.ones((), device=st.device)

    def path():
        ov, cboxes, cdescs = st.class_selector.select(proposals, sc["gt_dev"])
        scores, csel = m.class_branch(fm, list(cboxes))
        s, l = st.class_loss_selector(scores, csel, cdescs, ov, sc["gt_label"])
        torch.autograd.backward([st.class_criterion(s, l)], [one])
    t = timed(path, reps=50, warm=5)
    rows = int(st.class_out[0].shape[0])
    out.append(f"class path {label}: {len(proposals)} sample(s), {rows} forward boxes, level {tuple(int(v) for v in level.spatial_size)} "
               f"x {level.features.shape[1]} ch, {level.features.shape[0]} sites: draw + branch forward + loss + backward "
               f"{t:.3f} ms per call (50 back-to-back calls, host waits of the ROI cut included)")


def step_case(workload, dtype, n_gt, out, steps=10):
    from sparse_rcnn_amd.trainstep import SceneStep
    res = []
    for flags in (dict(), dict(class_loss=True, segmentation_loss=True)):
        st = SceneStep(workload, dtype=dtype, optimizer="adam", rpn_loss=True, mask_loss=True, n_gt=n_gt, prefetch=False,
                       lr=3e-5, **flags)
        for _ in range(3):
            st.step()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            st.step()
        b.record()
        torch.cuda.synchronize()
        st.finish()
        res.append(a.elapsed_time(b) / steps)
        del st
        torch.cuda.empty_cache()
    out.append(f"SceneStep {workload} {dtype} adam 3e-5 rpn_loss mask_loss" + (f" n_gt={n_gt}" if n_gt else "")
               + f": {res[0]:.3f} ms/step, {res[1]:.3f} ms/step with class_loss and segmentation_loss ({steps} steps)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-steps", action="store_true")
    args = ap.parse_args()
    out = [f"# class and segmentation losses on the device vs torch.nn.functional.cross_entropy ({torch.cuda.get_device_name(0)}); "
           "ms per call, device events around back-to-back calls through the Python API (host launch cost included)"]
    for n, c in ((172_500, 20), (600_000, 20), (96, 18), (480, 18)):
        xent_case(n, c, out)
    if not args.no_steps:
        class_path_case("cfg3-rpn", "cfg3-rpn", None, out)
        class_path_case("ref-crop-rpn n_gt=8", "ref-crop-rpn", 8, out)
        step_case("cfg3-rpn", "f32", None, out)
        step_case("ref-crop-rpn", "bf16", 8, out)
    text = "\n".join(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
