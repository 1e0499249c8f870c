"""The cfg2 training step (150 k voxels, U-Net 32-64-128-256) with the reference's other residual-unit forms -- bottleneck_divisor=4,
main_path_relu=True -- beside the default unit, the three alternating; and the closing ReLU of the main-path unit on its own:
the 14 in-place forward passes and the 14 masked backward passes of one step (two units in each of 4 encoder + 3 decoder
levels), timed on slabs of the step's own sizes.

    python tools/unit_forms_bench.py [--out profiles/unit_forms.txt] [--dtype f32|bf16] [--steps 20] [--rounds 3]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = (("default", {}), ("bottleneck_divisor=4", dict(bottleneck_divisor=4)), ("main_path_relu=True", dict(main_path_relu=True)))


def run_steps(st, steps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        st.step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def step_case(out, dtype, steps, rounds):
    from sparse_rcnn_amd.trainstep import SceneStep
    sts = {name: SceneStep("cfg2", dtype=dtype, lr=0.0, **kw) for name, kw in VARIANTS}
    for st in sts.values():
        for _ in range(5):
            st.step()
    res = {name: [] for name in sts}
    for _ in range(rounds):                                      # alternating
        for name, st in sts.items():
            res[name].append(run_steps(st, steps))
    for st in sts.values():
        st.finish()
    for name, st in sts.items():
        n_par = sum(p.numel() for p in st.model.parameters())
        out.append(f"SceneStep cfg2 {dtype} {name}: ms/step over {steps} steps per run " + " ".join(f"{v:.3f}" for v in res[name])
                   + f" (min {min(res[name]):.3f}); {n_par} parameters")
    unet = sts["main_path_relu=True"].model.backbone.unet
    rows = [int(t.features.shape[0]) for t in unet.interims]
    return rows, unet.channels


def relu_case(out, dtype, rows, channels, reps=50):
    """The closing ReLUs of one main-path step alone: per level l, 2 units x (encoder stage + decoder stage, the deepest level
    has no decoder stage) passes over a [rows_l, C_l] slab; forward in place, backward into a slab of its own."""
    from sparse_rcnn_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda")
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    fwd, bwd = (lib.scn_relu_fwd_bf16, lib.scn_relu_bwd_bf16) if dtype == "bf16" else (lib.scn_relu_fwd, lib.scn_relu_bwd)
    slabs = []
    for l, (n, c) in enumerate(zip(rows, channels)):
        for _ in range(2 * (2 if l + 1 < len(channels) else 1)):
            slabs.append((torch.randn(n, c, device=dev).to(tdt), torch.randn(n, c, device=dev).to(tdt),
                          torch.empty(n, c, device=dev, dtype=tdt)))

    def passes():
        for y, g, d in slabs:
            L.check(fwd(L.ptr(y), y.numel(), L.ptr(y), L.stream()))
        for y, g, d in slabs:
            L.check(bwd(L.ptr(y), L.ptr(g), y.numel(), L.ptr(d), L.stream()))
    for _ in range(5):
        passes()
    runs = []
    for _ in range(5):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            passes()
        b.record()
        torch.cuda.synchronize()
        runs.append(a.elapsed_time(b) / reps)
    es = 2 if dtype == "bf16" else 4
    traffic = sum(y.numel() for y, _, _ in slabs) * es * (2 + 3)          # forward: read + write; backward: two reads + write
    out.append(f"extra ReLU passes of a main_path_relu step alone, {dtype}: {len(slabs)} forward (in place) + {len(slabs)} backward "
               f"launches over the step's slabs (rows per level {rows}): ms per step " + " ".join(f"{v:.3f}" for v in runs)
               + f" (min {min(runs):.3f}); {traffic / 1e6:.1f} MB moved -> {traffic / min(runs) / 1e6:.0f} GB/s at the minimum, "
               "launched one by one through the Python API (inside a step the executor issues them from its C call)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", choices=("f32", "bf16"), nargs="*", default=["f32", "bf16"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    out = [f"# the cfg2 step with the reference's residual-unit forms ({torch.cuda.get_device_name(0)}); device events around "
           "back-to-back steps (index build, forward, backward, SGD update at lr 0), prefetch on"]
    for dtype in args.dtype:
        rows, channels = step_case(out, dtype, args.steps, args.rounds)
        relu_case(out, dtype, rows, channels)
    text = "\n".join(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
