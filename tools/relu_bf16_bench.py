"""Device time of the stand-alone ReLU on a bf16-stored slab and of the step it serves:

  1. scn_relu_fwd_bf16 / scn_relu_bwd_bf16 at the slab sizes of the reference's two dilation stacks (12 crops: 196 608 x 128 and
     24 576 x 256 elements) against scn_relu_fwd / scn_relu_bwd on the widened slab, in ms and GB/s (bytes read + written);
  2. SceneStep('ref-crop-rpn', upsample_heads=True, rpn_loss=True) in fp32, in bf16, and the 1x1 heads in bf16, alternating;
  3. with --parent DIR (a built checkout of the parent commit): the default `bench.py` there and here, alternating.

Medians of alternating rounds, inputs resident.

    python tools/relu_bf16_bench.py [--out profiles/anchor_up_bf16.txt] [--parent DIR] [--skip-steps]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from anchor_up_bench import Lines, rounds_line, timed            # noqa: E402  (tools/ is the script's directory)

SLABS = ((196608, 128), (24576, 256))


def kernels(lines, n_rounds):
    from sparse_rcnn_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    for rows, c in SLABS:
        n = rows * c
        xb = torch.randn(n, generator=g).to(dev).to(torch.bfloat16)
        gb = torch.randn(n, generator=g).to(dev).to(torch.bfloat16)
        xf, gf = xb.float(), gb.float()
        yb, yf = torch.empty_like(xb), torch.empty_like(xf)
        s = L.stream()
        calls = {
            "scn_relu_fwd_bf16": (lambda: lib.scn_relu_fwd_bf16(L.ptr(xb), n, L.ptr(yb), s), 2 * 2 * n),
            "scn_relu_fwd (widened slab)": (lambda: lib.scn_relu_fwd(L.ptr(xf), n, L.ptr(yf), s), 2 * 4 * n),
            "scn_relu_bwd_bf16": (lambda: lib.scn_relu_bwd_bf16(L.ptr(xb), L.ptr(gb), n, L.ptr(yb), s), 3 * 2 * n),
            "scn_relu_bwd (widened slab)": (lambda: lib.scn_relu_bwd(L.ptr(xf), L.ptr(gf), n, L.ptr(yf), s), 3 * 4 * n),
        }
        L.check(lib.scn_relu_fwd_bf16(L.ptr(xb), n, L.ptr(yb), s))
        L.check(lib.scn_relu_fwd(L.ptr(xf), n, L.ptr(yf), s))
        lines.append(f"slab {rows} x {c} = {n} elements ({2 * n / 1e6:.1f} MB bf16, {4 * n / 1e6:.1f} MB fp32); "
                     f"widen(relu_bf16(x)) == relu(widen(x)) bit for bit: {torch.equal(yb.float(), yf)}")
        t = {k: [] for k in calls}
        for _ in range(n_rounds):                                   # alternating
            for k, (fn, _) in calls.items():
                t[k].append(timed(fn, 50))
        for k, (_, moved) in calls.items():
            ms = statistics.median(t[k])
            lines.append(rounds_line(f"  {k}", t[k]) + f"; {moved / 1e6:.1f} MB read + written = {moved / ms / 1e6:.0f} GB/s")
    lines.append("(back-to-back launches between two events: each time holds the launch gap too, and a slab of 6 .. 100 MB "
                 "stays partly in the 256 MB Infinity Cache between repetitions -- these are not HBM rates)")


STEP_JOBS = (("fp32, up-sampling heads", dict(upsample_heads=True)),
             ("bf16, up-sampling heads", dict(upsample_heads=True, dtype="bf16")),
             ("bf16, 1x1 heads", dict(dtype="bf16")))


def steps(lines, n_rounds=3, n_steps=10):
    from sparse_rcnn_amd.trainstep import SceneStep
    jobs = {name: SceneStep("ref-crop-rpn", rpn_loss=True, **kw) for name, kw in STEP_JOBS}
    t = {name: [] for name in jobs}
    for job in jobs.values():
        for _ in range(3):
            job.step()
        job.finish()
    for _ in range(n_rounds):                                       # alternating
        for name, job in jobs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                job.step()
            job.finish()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3 / n_steps)
    for name in jobs:
        lines.append(rounds_line(f"SceneStep('ref-crop-rpn', rpn_loss=True) {name}, ms/step", t[name]))
    m = {name: statistics.median(v) for name, v in t.items()}
    a, b, c = (m[name] for name, _ in STEP_JOBS)
    lines.append(f"up-sampling heads: bf16 storage {b:.3f} ms/step against fp32 {a:.3f} ({a / b:.2f} x); against the 1x1 heads on "
                 f"bf16 storage {b - c:+.3f} ms ({100 * (b - c) / c:+.1f} %)")


def bench_pair(lines, parent, n_rounds=3, n_steps=50, warmup=10):
    def run(tree):
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(n_steps), "--warmup", str(warmup)],
                           cwd=tree, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"bench.py failed in {tree}: {r.stderr[-2000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    t = {"parent": [], "this change": []}
    for _ in range(n_rounds):                                       # alternating
        for name, tree in (("parent", parent), ("this change", ROOT)):
            t[name].append(float(run(tree)["ms_per_step"]))
            print(f"  [bench.py, {name}] {t[name][-1]:.4f} ms/step", flush=True)
    for name, v in t.items():
        lines.append(f"bench.py --gpus 1 --steps {n_steps} --warmup {warmup} (flagship cfg 2), {name}: ms_per_step "
                     f"{' '.join(f'{x:.4f}' for x in v)} (median {statistics.median(v):.4f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py there and here, alternating")
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    lines = Lines()
    kernels(lines, args.rounds)
    if not args.skip_steps:
        steps(lines, args.rounds)
        torch.cuda.empty_cache()
    if args.parent:
        torch.cuda.empty_cache()
        bench_pair(lines, args.parent)
    else:
        lines.append("bench.py parent against this change: NOT MEASURED in this run (no --parent tree given)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
