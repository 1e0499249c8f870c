"""Device time of the dense RoiAlign kernels (scn_roialign_fwd + scn_roialign_bwd behind functional.RoiAlignFunction) and of
the dense class branch end to end (classhead.DenseClassBranch forward + backward) at the reference's shape -- 12 crops, anchor
volume 32 x 32 x 16 x 128 at stride 4, R = 32 drawn proposals + 8 ground-truth boxes per crop, cut 16^3, 32 channels -- against
the restatement run as torch operators on the same device tensors (tests/roialign_restate.py: advanced indexing + weighted sum,
max_pool3d, conv3d, linear -- what the reference's dense arm executes).  Medians of alternating rounds, inputs resident.

--dtype bf16: the bf16-STORED forms (scn_roialign_fwd_bf16 / _bwd_bf16, scn_dense_maxpool_fwd_bf16 / _bwd_bf16,
DenseClassBranch(storage=torch.bfloat16)) at the same shape on bf16-valued inputs, with the fp32 forms re-measured on the
widened inputs in the alternating rounds of the same run (a comparison across runs would compare sessions); the torch
restatement is not timed again.

    python tools/roialign_bench.py [--dtype f32|bf16] [--out profiles/roialign.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12          # MI355X: bytes/s a streaming kernel reaches / the specification


def timed(fn, reps, warm=3):
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


def boxes_per_crop(rng, n, scene):
    scene = np.asarray(scene, np.float32)
    edge = rng.uniform(8, 96, (n, 3)).astype(np.float32).clip(max=scene)
    start = rng.uniform(0, 1, (n, 3)).astype(np.float32) * (scene - edge)
    return torch.from_numpy(np.stack([start, start + edge], 1))


def _rate(nbytes, ms):
    return (f"{nbytes / 1e6:.1f} MB in {ms:.4f} ms = {nbytes / ms / 1e9:.2f} TB/s = {100 * nbytes / ms / 1e-3 / HBM_ACHIEVABLE:.0f} % of "
            f"the 6.3 TB/s a streaming kernel reaches")


def bf16_against_f32(rounds):
    """-> the record's lines: every bf16 form next to its fp32 twin, alternating rounds of one run."""
    from sparse_rcnn_amd import roi
    from sparse_rcnn_amd.classhead import DenseClassBranch
    from sparse_rcnn_amd.functional import DenseMaxPoolFunction, RoiAlignFunction
    dev, bf = torch.device("cuda"), torch.bfloat16
    batch, size, stride, cut, c_vol, c = 12, (32, 32, 16), 4, (16, 16, 16), 128, 32
    rng = np.random.default_rng(0)
    bbox_batch = [boxes_per_crop(rng, 40, (128, 128, 64)).to(dev) for _ in range(batch)]
    bbox, counts, assoc = roi.transform_boxes_interpolation(bbox_batch, size, True, stride)
    r = bbox.shape[0]
    sample = assoc.to(dev, torch.int32)
    cells = batch * size[0] * size[1] * size[2]
    g = torch.Generator().manual_seed(0)
    lines = [f"shape: {batch} crops, volume {size[0]}x{size[1]}x{size[2]} cells at stride {stride}, R = {r} boxes (40 per crop, "
             f"edges 8-96 voxels), cut 16^3, {c} channels; intermediate [R*4096, {c}]: fp32 {r * 4096 * c * 4 / 1e6:.1f} MB, bf16 "
             f"{r * 4096 * c * 2 / 1e6:.1f} MB; inputs are bf16 values, the fp32 forms read them widened; medians of {rounds} "
             f"alternating rounds (f32, bf16, f32, ...), 20 launches per round"]
    med = lambda v: statistics.median(v)
    fmt = lambda v: " ".join(f"{x:.4f}" for x in v)

    # ---- the four kernels alone ----
    F16 = torch.randn((cells, c), generator=g).to(dev).to(bf)
    d16 = torch.randn((r * 4096, c), generator=g).to(dev).to(bf)
    ops = {}
    for name, F, dout in (("f32", F16.float(), d16.float()), ("bf16", F16, d16)):
        a = F.clone().requires_grad_()
        out = RoiAlignFunction.apply(a, bbox, sample, batch, size, cut)
        b = out.detach().clone().requires_grad_()
        pooled = DenseMaxPoolFunction.apply(b, r, cut)
        dpool = dout[:pooled.shape[0]].contiguous()

        def fwd(a=a):
            return RoiAlignFunction.apply(a, bbox, sample, batch, size, cut)

        def bwd(a=a, out=out, dout=dout):
            a.grad = None
            torch.autograd.backward([out], [dout], retain_graph=True)

        def pool_fwd(b=b):
            return DenseMaxPoolFunction.apply(b, r, cut)

        def pool_bwd(b=b, pooled=pooled, dpool=dpool):
            b.grad = None
            torch.autograd.backward([pooled], [dpool], retain_graph=True)

        es = F.element_size()
        ops[name] = dict(fwd=fwd, bwd=bwd, pool_fwd=pool_fwd, pool_bwd=pool_bwd, out=out, pooled=pooled,
                         bytes=dict(fwd=(out.numel() + F.numel()) * es, bwd=(dout.numel() + F.numel()) * es,
                                    pool_fwd=(out.numel() + pooled.numel()) * es + pooled.numel(),
                                    pool_bwd=(out.numel() + pooled.numel()) * es + pooled.numel()))
    same = torch.equal(ops["bf16"]["out"], ops["f32"]["out"].to(bf)) and torch.equal(ops["bf16"]["pooled"].float(), ops["f32"]["pooled"].to(bf).float())
    lines.append(f"bf16 forward == fp32 forward on the widened inputs, rounded once, and its max pool: {'equal bits' if same else 'DIFFERENT'}")
    t = {(k, n): [] for k in ("fwd", "bwd", "pool_fwd", "pool_bwd") for n in ("f32", "bf16")}
    for _ in range(rounds):
        for k in ("fwd", "bwd", "pool_fwd", "pool_bwd"):
            for n in ("f32", "bf16"):
                t[(k, n)].append(timed(ops[n][k], 20))
    what = {"fwd": "scn_roialign_fwd (output written once + volume read once)", "bwd": "scn_roialign_bwd (dOut read once + dF written once)",
            "pool_fwd": "scn_dense_maxpool_fwd (input read, output + argmax written)",
            "pool_bwd": "scn_dense_maxpool_bwd (dY + argmax read, dX written)"}
    for k in ("fwd", "bwd", "pool_fwd", "pool_bwd"):
        for n in ("f32", "bf16"):
            lines.append(f"{what[k]} {n}: {_rate(ops[n]['bytes'][k], med(t[(k, n)]))} (rounds {fmt(t[(k, n)])})")
        lines.append(f"  bf16 / f32 time: {med(t[(k, 'bf16')]) / med(t[(k, 'f32')]):.2f}")
    del ops

    # ---- the dense branch end to end ----
    torch.manual_seed(0)
    b32 = DenseClassBranch(c_vol, stride).to(dev)
    b16 = DenseClassBranch(c_vol, stride, storage=bf).to(dev)
    b16.load_state_dict(b32.state_dict())
    v16 = torch.randn((cells, c_vol), generator=g).to(dev).to(bf)
    gs = torch.randn((r, 18), generator=g).to(dev)

    def run(branch, vol):
        def f():
            vol.grad = None
            for p in branch.parameters():
                p.grad = None
            scores, _ = branch(vol, size, batch, bbox_batch)
            torch.autograd.backward([scores], [gs])
            return scores
        return f

    legs = {"fp32 branch, fp32 volume": run(b32, v16.float().requires_grad_()),
            "fp32 branch, bf16 volume widened on entry (the island of a bf16 step)": run(b32, v16.clone().requires_grad_()),
            "bf16-stored branch, bf16 volume": run(b16, v16.clone().requires_grad_())}
    s = {k: f().detach() for k, f in legs.items()}
    keys = list(legs)
    lines.append(f"dense branch, scores bf16-stored vs fp32: max diff {float((s[keys[2]] - s[keys[0]]).abs().max()):.2e} "
                 f"(scale {float(s[keys[0]].abs().max()):.3g})")
    tb = {k: [] for k in legs}
    for _ in range(rounds):
        for k, f in legs.items():
            tb[k].append(timed(f, 5, 2))
    for k in keys:
        lines.append(f"dense branch fwd + bwd (R = {r}, bucket {b32.bucket(r)}), {k}: median {med(tb[k]):.3f} ms (rounds "
                     f"{' '.join(f'{x:.3f}' for x in tb[k])})")
    lines.append(f"  bf16-stored / fp32 island: {med(tb[keys[2]]) / med(tb[keys[1]]):.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    args = ap.parse_args()
    if args.dtype == "bf16":
        text = "\n".join(bf16_against_f32(args.rounds))
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    import roialign_restate as R
    from sparse_rcnn_amd import roi
    from sparse_rcnn_amd.classhead import DenseClassBranch, slab_to_conv3d_weight
    from sparse_rcnn_amd.functional import RoiAlignFunction
    dev = torch.device("cuda")
    batch, size, stride, cut, c_vol, c = 12, (32, 32, 16), 4, (16, 16, 16), 128, 32
    rng = np.random.default_rng(0)
    bbox_batch = [boxes_per_crop(rng, 40, (128, 128, 64)).to(dev) for _ in range(batch)]
    bbox, counts, assoc = roi.transform_boxes_interpolation(bbox_batch, size, True, stride)
    r = bbox.shape[0]
    sample = assoc.to(dev, torch.int32)
    cells = batch * size[0] * size[1] * size[2]
    g = torch.Generator().manual_seed(0)
    F32 = torch.randn((cells, c), generator=g).to(dev)
    dout = torch.randn((r * 4096, c), generator=g).to(dev)
    lines = [f"shape: {batch} crops, volume {size[0]}x{size[1]}x{size[2]} cells at stride {stride}, R = {r} boxes (40 per crop, "
             f"edges 8-96 voxels), cut 16^3, {c} channels; intermediate [R*4096, {c}] fp32 = {r * 4096 * c * 4 / 1e6:.1f} MB"]

    # ---- the two kernels alone ----
    a = F32.clone().requires_grad_()

    def ours_fwd():
        return RoiAlignFunction.apply(a, bbox, sample, batch, size, cut)

    out = ours_fwd()

    def ours_bwd():
        a.grad = None
        torch.autograd.backward([out], [dout], retain_graph=True)

    vol5 = F32.view(batch, *size, c).clone().requires_grad_()

    def ref_fwd():
        return R.roialign(vol5, bbox, assoc.to(dev), cut)

    def ref_both():
        vol5.grad = None
        torch.autograd.backward([ref_fwd()], [dout.view(r, 16, 16, 16, c)])

    t = {"fwd": [], "bwd": [], "ref_fwd": [], "ref_both": []}
    for _ in range(args.rounds):                                  # alternating
        t["fwd"].append(timed(ours_fwd, 20))
        t["ref_fwd"].append(timed(ref_fwd, 3, 1))
        t["bwd"].append(timed(ours_bwd, 20))
        t["ref_both"].append(timed(ref_both, 3, 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    fwd_bytes = out.numel() * 4 + F32.numel() * 4
    bwd_bytes = dout.numel() * 4 + F32.numel() * 4
    for k, v in t.items():
        lines.append(f"{k}: median {med[k]:.4f} ms (rounds {' '.join(f'{x:.4f}' for x in v)})")
    lines.append(f"scn_roialign_fwd: {fwd_bytes / 1e6:.1f} MB (output written once + volume read once) in {med['fwd']:.4f} ms = "
                 f"{fwd_bytes / med['fwd'] / 1e9:.2f} TB/s = {100 * fwd_bytes / med['fwd'] / 1e-3 / HBM_ACHIEVABLE:.0f} % of the 6.3 TB/s "
                 f"a streaming kernel reaches ({100 * fwd_bytes / med['fwd'] / 1e-3 / HBM_PEAK:.0f} % of the 8 TB/s peak)")
    lines.append(f"scn_roialign_bwd: {bwd_bytes / 1e6:.1f} MB (dOut read once + dF written once) in {med['bwd']:.4f} ms = "
                 f"{bwd_bytes / med['bwd'] / 1e9:.2f} TB/s = {100 * bwd_bytes / med['bwd'] / 1e-3 / HBM_ACHIEVABLE:.0f} % of 6.3 TB/s")
    lines.append(f"kernels fwd + bwd {med['fwd'] + med['bwd']:.4f} ms against the restatement's {med['ref_both']:.4f} ms "
                 f"({med['ref_both'] / (med['fwd'] + med['bwd']):.1f} x)")
    del out, vol5

    # ---- the dense branch end to end ----
    torch.manual_seed(0)
    branch = DenseClassBranch(c_vol, stride).to(dev)
    vol = torch.randn((cells, c_vol), generator=g).to(dev).requires_grad_()
    gs = torch.randn((r, 18), generator=g).to(dev)
    sd = {}
    own = branch.named_oracle_params()
    for rk, name in branch.reference_key_map().items():
        p = own[name].detach()
        sd[rk] = (slab_to_conv3d_weight(p, round(p.shape[0] ** (1 / 3))).contiguous() if p.dim() == 3 else p.clone()).requires_grad_()
    vol_ncxyz = vol.detach().view(batch, *size, c_vol).permute(0, 4, 1, 2, 3).contiguous().requires_grad_()

    def ours():
        vol.grad = None
        for p in branch.parameters():
            p.grad = None
        scores, _ = branch(vol, size, batch, bbox_batch)
        torch.autograd.backward([scores], [gs])
        return scores

    def theirs():
        vol_ncxyz.grad = None
        for p in sd.values():
            p.grad = None
        scores, _, _ = R.dense_class_forward(sd, vol_ncxyz, bbox_batch, float(stride), cut)
        torch.autograd.backward([scores], [gs])
        return scores

    s_a, s_b = ours().detach(), theirs().detach()
    lines.append(f"dense branch, scores ours vs restatement: max diff {float((s_a - s_b).abs().max()):.2e} (scale {float(s_b.abs().max()):.3g})")
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(timed(ours, 5, 2))
        tb.append(timed(theirs, 3, 1))
    lines.append(f"dense branch fwd + bwd (R = {r}, bucket {branch.bucket(r)}): median {statistics.median(ta):.3f} ms (rounds "
                 f"{' '.join(f'{x:.3f}' for x in ta)}); restatement on torch operators {statistics.median(tb):.3f} ms (rounds "
                 f"{' '.join(f'{x:.3f}' for x in tb)}): {statistics.median(tb) / statistics.median(ta):.1f} x")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
