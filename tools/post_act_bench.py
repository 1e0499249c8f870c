"""The cfg2 training step (150 k voxels, U-Net 32-64-128-256) with the reference's post-activation units (relu_first=False), with
the input-stage ReLUs kept (drop_input_relu=False) and with plain convolution blocks (use_residuals=False), beside the default
of the same build, the variants alternating; and the fused end of a post-activation unit, SCN_OP_ADD_RELU as a one-op executor plan (y = x +
max(x1, 0), 3 slab passes), against the two launches it replaces, scn_relu_fwd + scn_add (5 slab passes), at cfg2's level-0 shape.

    python tools/post_act_bench.py [--out profiles/post_act.txt] [--dtype f32|bf16] [--steps 20] [--rounds 3]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = (("default", {}), ("relu_first=False", dict(relu_first=False)),
            ("relu_first=False, drop_input_relu=False", dict(relu_first=False, drop_input_relu=False)),
            ("drop_input_relu=False", dict(drop_input_relu=False)),
            ("use_residuals=False", dict(use_residuals=False)),
            ("use_residuals=False, relu_first=False", dict(use_residuals=False, relu_first=False)))


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
    unet = sts["default"].model.backbone.unet
    return int(unet.interims[0].features.shape[0]), unet.channels[0]


def add_relu_case(out, dtype, n, c, reps=200):
    """One unit's end at level 0: the fused launch against the pair, on slabs of their own, alternating."""
    from sparse_rcnn_amd import _lib as L, executor as EX
    lib = L.lib()
    dev = torch.device("cuda")
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    relu, add = (lib.scn_relu_fwd_bf16, lib.scn_add_bf16) if dtype == "bf16" else (lib.scn_relu_fwd, lib.scn_add)
    scratch = torch.empty(256, dtype=torch.uint8, device=dev)
    x, t = torch.randn(n, c, device=dev).to(tdt), torch.randn(n, c, device=dev).to(tdt)
    r, y = torch.empty_like(x), torch.empty_like(x)
    cnt, s = x.numel(), L.stream()

    def one():
        EX.run_add_relu(L.ptr(x), L.ptr(t), L.ptr(y), n, c, dtype == "bf16", scratch)

    def two():
        L.check(relu(L.ptr(t), cnt, L.ptr(r), s))
        L.check(add(L.ptr(x), L.ptr(r), cnt, L.ptr(y), s))
    runs = {"fused": [], "pair": []}
    for fn in (one, two):
        for _ in range(10):
            fn()
    for _ in range(5):
        for name, fn in (("fused", one), ("pair", two)):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            runs[name].append(a.elapsed_time(b) / reps * 1e3)
    es = 2 if dtype == "bf16" else 4
    f, p = min(runs["fused"]), min(runs["pair"])
    med = sorted(runs["pair"])[2] / sorted(runs["fused"])[2]
    out.append(f"end of a post-activation unit at level 0, {dtype}, [{n}, {c}] slabs, back-to-back launches through the Python API: "
               f"SCN_OP_ADD_RELU (one-op scn_exec_run) us " + " ".join(f"{v:.1f}" for v in runs["fused"]) + f" (min {f:.1f}, {3 * cnt * es / f / 1e3:.0f} GB/s over 3 "
               f"passes); scn_relu_fwd + scn_add us " + " ".join(f"{v:.1f}" for v in runs["pair"])
               + f" (min {p:.1f}, {5 * cnt * es / p / 1e3:.0f} GB/s over 5 passes); pair / fused = {p / f:.2f} at the minima, {med:.2f} at the medians (by traffic 5 / 3 = 1.67); "
               f"the three slabs ({3 * cnt * es / 1e6:.0f} MB) stay in the last-level cache between launches, so these are not HBM rates")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", choices=("f32", "bf16"), nargs="*", default=["f32", "bf16"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    out = [f"# the cfg2 step with the reference's post-activation units, input-stage ReLUs and plain blocks "
           f"({torch.cuda.get_device_name(0)}); device events around back-to-back steps (index build, forward, backward, SGD update "
           "at lr 0), prefetch on"]
    for dtype in args.dtype:
        n, c = step_case(out, dtype, args.steps, args.rounds)
        add_relu_case(out, dtype, n, c)
    text = "\n".join(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
