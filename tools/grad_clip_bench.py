"""What global-norm gradient clipping (SceneStep(max_grad_norm=), executor ops SCN_OP_GRAD_NORM / SCN_OP_GRAD_SCALE) costs.
    python tools/grad_clip_bench.py [--blocks 4] [--steps 25] [--warmup 10] [--dtypes f32 bf16] [--elements 14000000]
                                    [--reps 200] [--lr 0] [--out profiles/grad_clip.txt]

1. The cfg2 step with Adam in ONE process, three variants built first and alternated block by block (event-timed ms/step):
   the default (no clipping: nothing is built or launched), max_grad_norm=1e30 (the norm is computed, the scale launch returns at
   its first load) and a bound far below the norm (every step is clipped).  --lr defaults to 0: the update launch does the same
   work and the weights stay as initialised (at the reference's 4e-4 the same synthetic N(0, 1) gradient on every output, step
   after step, drives this workload's activations out of range within a hundred steps, and a non-finite norm is all there is to
   read -- a first run of this tool showed it).
2. The two ops alone on an fp32 buffer of --elements values, HIP events around --reps back-to-back executor calls: the norm alone
   (bound +inf), and norm + scale with a coefficient below 1 in the record the scale op reads (a record of its own, so that the
   buffer shrinks by 1e-7 per call and every call does the full work).  Once on ONE buffer, which stays in the 256 MB last-level
   cache between calls, and once rotating over enough buffers to exceed it: the second is the HBM figure.  The yardstick is the
   byte count: 4 B per element read for the norm, 8 B per element more (read + write) when clipping, against the streaming rate
   profiles/adam_bw.txt records for the Adam kernel.
Without a GPU the command parses its arguments, lists what it would measure and measures nothing."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def timed_block(fn, steps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def steps_case(dtype, args, say):
    from sparse_rcnn_amd.trainstep import SceneStep
    dev = torch.device("cuda", 0)
    variants = {"default": None, "norm only (1e30)": 1e30, "clips (1e-3)": 1e-3}
    jobs = {k: SceneStep("cfg2", dev, dtype=dtype, optimizer="adam", lr=args.lr, max_grad_norm=v) for k, v in variants.items()}
    for job in jobs.values():
        for _ in range(args.warmup):
            job.step()
        job.finish()
    ms = {k: [] for k in jobs}
    for _ in range(args.blocks):                       # the variants alternate block by block: drift hits all alike
        for name, job in jobs.items():
            ms[name].append(timed_block(job.step, args.steps))
            job.finish()
    first = next(iter(jobs.values()))
    say(f"== cfg2 {dtype}, Adam: {first.n_active} active voxels, {len(first.flat.params)} parameter tensors, "
        f"{first.flat.flat.numel()} parameters, lr {args.lr:g}; {args.blocks} blocks of {args.steps} steps after {args.warmup} warm-up steps ==")
    base = ms["default"]
    for name, job in jobs.items():
        v = ms[name]
        extra = "" if name == "default" else ("   minus default per block (us): "
                                              + " ".join(f"{1e3 * (a - b):7.1f}" for a, b in zip(v, base)))
        gn = job.grad_norm
        rec = "" if gn is None else f"   last record: norm {gn[0]:.4g}, coefficient {gn[1]:.4g}, nonfinite {gn[2]}"
        say(f"  {name:18s} ms/step per block: " + " ".join(f"{x:7.3f}" for x in v) + f"   median {sorted(v)[len(v) // 2]:.3f}"
            + extra + rec)
    del jobs
    torch.cuda.empty_cache()


def ops_case(args, say):
    from sparse_rcnn_amd import _lib as L, executor as EX
    dev = torch.device("cuda", 0)
    n = args.elements
    lib = L.lib()
    scratch = torch.empty(EX.clip_scratch_bytes([n]), dtype=torch.uint8, device=dev)
    rec = torch.zeros(4, device=dev)
    fixed = torch.tensor([0.0, 1.0 - 2.0 ** -23, 0.0, 0.0], device=dev)        # a coefficient just below 1: the scale op always works
    table = (C.c_void_p * 2)(rec.data_ptr(), fixed.data_ptr())

    def plan(x1):
        ops, levels, prefix = EX.clip_plan([n], float("inf"), 1.0)
        ops[1].x1 = x1
        return ops, levels, prefix
    plans = {"norm alone (scale returns at once)": (plan(0), 4), "norm + scale": (plan(1), 12)}
    for label, n_buf in (("ONE buffer (stays in the last-level cache)", 1),
                         (f"rotating over {args.rotate} buffers ({args.rotate * n * 4 / 2**20:.0f} MiB: HBM)", args.rotate)):
        bufs = [torch.randn(n, device=dev) for _ in range(n_buf)]
        grads = [(C.c_void_p * 1)(b.data_ptr()) for b in bufs]
        say(f"== the ops alone, {n} fp32 elements ({n * 4 / 1e6:.1f} MB), {args.reps} back-to-back one-call plans, {label} ==")
        for name, ((ops, levels, prefix), bytes_per) in plans.items():
            k = [0]

            def call():
                g = grads[k[0] % n_buf]
                k[0] += 1
                L.check(lib.scn_exec_run(ops, 2, levels, 1, table, None, g, scratch.data_ptr(), scratch.numel(), None, L.stream()))
            for _ in range(10):
                call()
            us = [1e3 * timed_block(call, args.reps) for _ in range(5)]
            best = min(us)
            say(f"  {name:36s} us per call " + " ".join(f"{v:6.1f}" for v in us) + f"   min {best:.1f}: {bytes_per} B/element -> "
                f"{bytes_per * n / best / 1e6:.2f} TB/s; at the 6.4 TB/s of scn_adam_many on this chip (profiles/adam_bw.txt) the bytes "
                f"alone take {bytes_per * n / 6.4e6:.1f} us: measured / estimated = {best / (bytes_per * n / 6.4e6):.2f} "
                "(3 launches per call)")
        del bufs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--lr", type=float, default=0.0)
    ap.add_argument("--elements", type=int, default=14_000_000)
    ap.add_argument("--rotate", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if not torch.cuda.is_available():
        for d in args.dtypes:
            print(f"would measure SceneStep('cfg2', dtype={d!r}, optimizer='adam') against max_grad_norm=1e30 and max_grad_norm=1e-3")
        print(f"would measure SCN_OP_GRAD_NORM and SCN_OP_GRAD_SCALE alone on {args.elements} fp32 elements")
        print("no GPU: nothing measured")
        return
    say(f"# tools/grad_clip_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    for d in args.dtypes:
        steps_case(d, args, say)
    ops_case(args, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
