"""The joint training step (all four losses, every part trainable) against the mask-only stage, `train=("mask",)` with the same
switches, in ONE process: event-timed milliseconds per step in alternating blocks, peak allocated bytes, and library calls that
launch kernels per step.
    python tools/train_parts_bench.py [--blocks 4] [--steps 10] [--warmup 5] [--workloads cfg3-rpn ref-crop-rpn]
                                      [--dtypes f32 bf16] [--lr 0] [--out profiles/train_parts.txt]

Both steps are built first and stay resident, so each block of either variant sees the same resident tensors; the peak is
`torch.cuda.max_memory_allocated` over a variant's blocks after `reset_peak_memory_stats` at each block's start.  Calls are counted
by tools/call_count.py: every launching entry point called from Python, plus one per op of every `scn_exec_run*`
plan (scn_exec_timing_enable(2) records one entry per op).  `forward_only` of the joint step's model (the evaluation forward:
index build + backbone + RPN + mask branch under no_grad) is timed beside them for orientation.
--lr defaults to 0: the update launch does the same work and the weights stay as initialised, so both variants select the same
proposals and crop the same points in every step (with a learning rate the joint step's RPN moves and the two crops drift apart).
Without a GPU the command parses its arguments, lists what it would measure and measures nothing."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from call_count import counted, launching_calls
from sparse_rcnn_amd.trainstep import SceneStep

FOUR = dict(rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True)
WORKLOADS = {"cfg3-rpn": dict(), "ref-crop-rpn": dict(upsample_heads=True, dense_class=True, n_gt=8)}


def timed_block(fn, steps):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps, torch.cuda.max_memory_allocated()


def measure(workload, dtype, args, say):
    dev = torch.device("cuda", 0)
    kw = dict(dtype=dtype, optimizer="adam", lr=args.lr, **FOUR, **WORKLOADS[workload])
    jobs = {"joint": SceneStep(workload, dev, **kw), "mask-only": SceneStep(workload, dev, train=("mask",), **kw)}
    for job in jobs.values():
        for _ in range(args.warmup):
            job.step()
        job.finish()
    joint = jobs["joint"]
    for _ in range(args.warmup):
        joint.forward_only()
    joint.finish()
    ms = {k: [] for k in (*jobs, "forward_only")}
    peak = {k: 0 for k in ms}
    for _ in range(args.blocks):                   # the variants alternate block by block: drift hits both alike
        for name, job in jobs.items():
            t, p = timed_block(job.step, args.steps)
            job.finish()
            ms[name].append(t)
            peak[name] = max(peak[name], p)
        t, p = timed_block(joint.forward_only, args.steps)
        joint.finish()
        ms["forward_only"].append(t)
        peak["forward_only"] = max(peak["forward_only"], p)
    resident = torch.cuda.memory_allocated()
    say(f"== {workload} {dtype}: {joint.n_active} active voxels, {args.blocks} blocks of {args.steps} steps after {args.warmup} warm-up "
        f"steps, Adam lr {args.lr:g}; {resident / 2**20:.0f} MiB resident between blocks (both steps) ==")
    for name, job in jobs.items():
        calls, runs, ops = launching_calls(*counted(job.step))
        job.finish()
        say(f"  {name:12s} ms/step per block: " + " ".join(f"{v:8.3f}" for v in ms[name])
            + f"   peak allocated {peak[name] / 2**20:8.0f} MiB   {calls:5d} launching calls/step ({runs} executor passes holding {ops} ops)"
            + f"   {len(job.flat.params)} parameter tensors, {job.flat.flat.numel()} values in the optimizer; {job.n_roi_rows} cropped points")
    say(f"  {'forward_only':12s} ms/step per block: " + " ".join(f"{v:8.3f}" for v in ms["forward_only"])
        + f"   peak allocated {peak['forward_only'] / 2**20:8.0f} MiB   (the joint step's model under no_grad, for orientation)")
    faster = [b < a for a, b in zip(ms["joint"], ms["mask-only"])]
    say(f"  mask-only faster than joint in {sum(faster)} of {len(faster)} blocks; ratio per block "
        + " ".join(f"{b / a:.3f}" for a, b in zip(ms["joint"], ms["mask-only"]))
        + f"; peak allocation {'lower' if peak['mask-only'] < peak['joint'] else 'NOT lower'} "
        f"({(peak['joint'] - peak['mask-only']) / 2**20:.0f} MiB less)")
    del jobs, joint
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.0)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if not torch.cuda.is_available():
        for w in args.workloads:
            for d in args.dtypes:
                print(f"would measure SceneStep({w!r}, dtype={d!r}, optimizer='adam', four losses"
                      + "".join(f", {k}={v!r}" for k, v in WORKLOADS[w].items()) + ") against the same with train=('mask',)")
        print("no GPU: nothing measured")
        return
    say(f"train_parts_bench on {torch.cuda.get_device_name(0)}: joint step (rpn + class + mask + segmentation losses, every part "
        "trainable) against train=('mask',), one process, variants alternated")
    for w in args.workloads:
        for d in args.dtypes:
            measure(w, d, args, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
