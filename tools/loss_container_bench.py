"""The loss container (loss.Loss.combine: scn_loss_combine forward, scn_loss_combine_bwd backward) against the same arithmetic
written in torch operations on device scalars -- the reference's loss.py:101-191 without its `.item()` calls; that restatement
lives here only --, the two alternating; then the cfg3-rpn step with all four losses, multitask_loss on and off, alternating.

    python tools/loss_container_bench.py [--out profiles/loss_container.txt] [--no-steps]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 200
NEEDED = dict(mask_positive_threshold=0.2, class_positive_threshold=0.1, class_negative_threshold=0, class_negative_label=-100)


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


def launches(fn):
    """Device kernels of one call, counted by torch's profiler (None where it does not report them)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:          # noqa: BLE001  (a profiler that is not there is not this tool's subject)
        return None


def torch_form(terms, w, default):
    """loss.py:101-191 on device scalars: every term present, the RPN weights crossed as the reference writes them."""
    loss = default.clone()
    extra = default.clone()
    loss += terms[0] * torch.exp(-w[1])
    loss += terms[1] * torch.exp(-w[0])
    extra += w[1]
    extra += w[0]
    for i in (2, 3, 4):
        loss += terms[i] * torch.exp(-w[i])
        extra += w[i]
    return loss + extra, loss


def combine_case(out, rounds=5):
    from sparse_rcnn_amd.loss import Loss
    dev = torch.device("cuda")
    crit = Loss(batchwise_subsample=True, sparse=True, multitask_loss=True, loss_rpn_class_weight=2, loss_rpn_bbox_weight=0.5,
                loss_class_weight=0.25, loss_mask_weight=4, loss_segmentation_weight=0.125, calc_bbox=True, calc_class=True,
                calc_mask=True, calc_segmentation=True, **NEEDED).to(dev)
    terms = [torch.tensor(v, device=dev).requires_grad_() for v in (0.71, 0.052, 2.9, 0.64, 3.0)]
    w = crit.log_weights()
    one = torch.ones((), device=dev)

    def drop():
        for t in terms + w:
            t.grad = None

    def ours():
        drop()
        torch.autograd.backward([crit.combine(terms)[0]], [one])

    def theirs():
        drop()
        torch.autograd.backward([torch_form(terms, w, crit.default_loss)[0]], [one])

    ours()
    mine = [float(t.grad) for t in terms + w]
    theirs()
    ref = [float(t.grad) for t in terms + w]
    worst = max(abs(a - b) / max(abs(b), 1e-30) for a, b in zip(mine, ref))
    a, b = [], []
    for _ in range(rounds):                                      # alternating
        a.append(timed(ours))
        b.append(timed(theirs))
    na, nb = launches(ours), launches(theirs)
    ma, mb = sorted(a)[len(a) // 2], sorted(b)[len(b) // 2]
    out.append(f"container fwd+bwd, 5 terms, multitask_loss: device min {min(a) * 1e3:.1f} median {ma * 1e3:.1f} us (runs "
               f"{' '.join(f'{v * 1e3:.1f}' for v in a)}), torch form min {min(b) * 1e3:.1f} median {mb * 1e3:.1f} us (runs "
               f"{' '.join(f'{v * 1e3:.1f}' for v in b)}), torch / device {min(b) / min(a):.2f}x (min), {mb / ma:.2f}x (median); "
               f"{REPS} repetitions per run; kernel launches per call: device {na if na is not None else 'not counted'} "
               f"(by construction 2: k_loss_combine, k_loss_combine_bwd), torch form {nb if nb is not None else 'not counted'}; "
               f"largest relative difference of the ten gradients {worst:.2e}")


def step_case(out, steps=10, rounds=3):
    from sparse_rcnn_amd.trainstep import SceneStep
    kw = dict(optimizer="adam", lr=3e-5, rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True, prefetch=False)
    sts = {"off": SceneStep("cfg3-rpn", **kw), "on": SceneStep("cfg3-rpn", multitask_loss=True, **kw)}
    res = {k: [] for k in sts}
    for st in sts.values():
        for _ in range(3):
            st.step()
    for _ in range(rounds):                                      # alternating
        for name, st in sts.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                st.step()
            b.record()
            torch.cuda.synchronize()
            res[name].append(a.elapsed_time(b) / steps)
    for st in sts.values():
        st.finish()
    weights = sts["on"].loss_weights()
    out.append("SceneStep cfg3-rpn f32 adam 3e-5, all four losses, ms/step over " + f"{steps} steps per run: multitask_loss off "
               + " ".join(f"{v:.3f}" for v in res["off"]) + ", on " + " ".join(f"{v:.3f}" for v in res["on"])
               + f"; weights after {3 + rounds * steps} steps: " + ", ".join(f"{k} {v:.5f}" for k, v in weights.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-steps", action="store_true")
    args = ap.parse_args()
    out = [f"# the loss container against its torch formulation ({torch.cuda.get_device_name(0)}); device events around "
           "back-to-back calls through the Python API (host launch cost included)"]
    combine_case(out)
    if not args.no_steps:
        step_case(out)
    text = "\n".join(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
