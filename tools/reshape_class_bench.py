"""Device time of RoiAlign + max pool as ONE pass (scn_roialign_pool_fwd / _bwd behind functional.RoiAlignPoolFunction) against
the two-call chain (RoiAlignFunction + DenseMaxPoolFunction), at the shape of tools/roialign_bench.py -- 12 crops, anchor volume
32 x 32 x 16 at stride 4, 480 boxes drawn the same way -- in three settings, all in ONE run, medians of alternating rounds,
inputs resident:

  (a) the kernels alone at the reshaping class head's shape: C = 128, cut 8^3 -- forward, backward and the bytes each side
      moves, fp32 and bf16-stored;
  (b) classhead.ReshapeClassBranch forward + backward, fused on and off;
  (c) classhead.DenseClassBranch at its own shape (C = 32 behind its input convolution, cut 16^3), fused_pool on and off.

    python tools/reshape_class_bench.py [--rounds 5] [--out profiles/reshape_class.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from roialign_bench import boxes_per_crop, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    from sparse_rcnn_amd import roi
    from sparse_rcnn_amd.classhead import DenseClassBranch, ReshapeClassBranch
    from sparse_rcnn_amd.functional import DenseMaxPoolFunction, RoiAlignFunction, RoiAlignPoolFunction
    dev, bf = torch.device("cuda"), torch.bfloat16
    batch, size, stride, cut, c = 12, (32, 32, 16), 4, (8, 8, 8), 128
    rng = np.random.default_rng(0)
    bbox_batch = [boxes_per_crop(rng, 40, (128, 128, 64)).to(dev) for _ in range(batch)]
    bbox, counts, assoc = roi.transform_boxes_interpolation(bbox_batch, size, True, stride)
    r = bbox.shape[0]
    sample = assoc.to(dev, torch.int32)
    cells = batch * size[0] * size[1] * size[2]
    g = torch.Generator().manual_seed(0)
    med = statistics.median
    fmt = lambda v: " ".join(f"{x:.4f}" for x in v)
    lines = [f"shape: {batch} crops, volume {size[0]}x{size[1]}x{size[2]} cells at stride {stride}, R = {r} boxes (40 per crop, "
             f"edges 8-96 voxels); medians of {args.rounds} alternating rounds (chain, fused, chain, ...) of one run"]

    # ---- (a) the kernels alone: C = 128, cut 8^3 ----
    n_cut, n_pool = r * 512, r * 64
    F16 = torch.randn((cells, c), generator=g).to(dev).to(bf)
    d16 = torch.randn((n_pool, c), generator=g).to(dev).to(bf)
    lines.append(f"(a) C = {c}, cut 8^3: un-pooled samples [R*512, {c}] = {n_cut * c * 4 / 1e6:.1f} MB fp32 / {n_cut * c * 2 / 1e6:.1f} MB "
                 f"bf16; pooled [R*64, {c}] = {n_pool * c * 4 / 1e6:.1f} / {n_pool * c * 2 / 1e6:.1f} MB (+ {n_pool * c / 1e6:.1f} MB argmax); "
                 f"volume {cells * c * 4 / 1e6:.1f} / {cells * c * 2 / 1e6:.1f} MB")
    for name, F, dy in (("f32", F16.float(), d16.float()), ("bf16", F16, d16)):
        es = F.element_size()
        a0, a1 = F.clone().requires_grad_(), F.clone().requires_grad_()

        def chain_fwd(a0=a0):
            return DenseMaxPoolFunction.apply(RoiAlignFunction.apply(a0, bbox, sample, batch, size, cut), r, cut)

        def fused_fwd(a1=a1):
            return RoiAlignPoolFunction.apply(a1, bbox, sample, batch, size, cut)

        y0, y1 = chain_fwd(), fused_fwd()

        def chain_bwd(a0=a0, y0=y0, dy=dy):
            a0.grad = None
            torch.autograd.backward([y0], [dy], retain_graph=True)

        def fused_bwd(a1=a1, y1=y1, dy=dy):
            a1.grad = None
            torch.autograd.backward([y1], [dy], retain_graph=True)

        chain_bwd(); fused_bwd()
        same = torch.equal(y0.view(torch.int16 if es == 2 else torch.int32), y1.view(torch.int16 if es == 2 else torch.int32))
        lines.append(f"  {name}: fused forward {'== chain, equal bits' if same else 'DIFFERS from the chain'}; backward "
                     f"{'equal' if torch.equal(a0.grad, a1.grad) else 'DIFFERENT'}")
        # bytes each side must move (every buffer once): volume + samples written, samples re-read, pooled + argmax written
        moved = {"chain_fwd": (cells * c + 2 * n_cut * c + n_pool * c) * es + n_pool * c,
                 "fused_fwd": (cells * c + n_pool * c) * es + n_pool * c,
                 "chain_bwd": (n_pool * c + 2 * n_cut * c + cells * c) * es + n_pool * c,
                 "fused_bwd": (n_pool * c + cells * c) * es + n_pool * c}
        t = {k: [] for k in moved}
        legs = dict(chain_fwd=chain_fwd, fused_fwd=fused_fwd, chain_bwd=chain_bwd, fused_bwd=fused_bwd)
        for _ in range(args.rounds):
            for k in ("chain_fwd", "fused_fwd", "chain_bwd", "fused_bwd"):
                t[k].append(timed(legs[k], 20))
        for d in ("fwd", "bwd"):
            tc, tf = med(t["chain_" + d]), med(t["fused_" + d])
            lines.append(f"  {name} {d}: chain {tc:.4f} ms moving {moved['chain_' + d] / 1e6:.1f} MB (rounds {fmt(t['chain_' + d])}); "
                         f"fused {tf:.4f} ms moving {moved['fused_' + d] / 1e6:.1f} MB (rounds {fmt(t['fused_' + d])}); "
                         f"fused / chain time {tf / tc:.2f}")
        del a0, a1, y0, y1

    # ---- (b), (c): the branches end to end ----
    def run(branch, vol, gs):
        def f():
            vol.grad = None
            for p in branch.parameters():
                p.grad = None
            scores, _ = branch(vol, size, batch, bbox_batch)
            torch.autograd.backward([scores], [gs])
            return scores
        return f

    gs = torch.randn((r, 18), generator=g).to(dev)
    vol = torch.randn((cells, c), generator=g).to(dev)
    verdict = None
    for tag, make, what in (
            ("(b)", lambda fused: ReshapeClassBranch(c, stride, fused=fused), "ReshapeClassBranch (C = 128, cut 8^3, same-conv 128->8), fused"),
            ("(c)", lambda fused: DenseClassBranch(c, stride, fused_pool=fused), "DenseClassBranch (C = 32 behind its input convolution, cut 16^3), fused_pool")):
        torch.manual_seed(0)
        off = make(False).to(dev)
        on = make(True).to(dev)
        on.load_state_dict(off.state_dict())
        legs = {"off": run(off, vol.clone().requires_grad_(), gs), "on": run(on, vol.clone().requires_grad_(), gs)}
        s = {k: f().detach() for k, f in legs.items()}
        t = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, f in legs.items():
                t[k].append(timed(f, 5, 2))
        ratio = med(t["on"]) / med(t["off"])
        lines.append(f"{tag} {what} off / on, fwd + bwd (R = {r}, bucket {off.bucket(r)}): scores "
                     f"{'equal bits' if torch.equal(s['on'].view(torch.int32), s['off'].view(torch.int32)) else 'DIFFERENT'}; off "
                     f"{med(t['off']):.3f} ms (rounds {fmt(t['off'])}); on {med(t['on']):.3f} ms (rounds {fmt(t['on'])}); on / off {ratio:.2f}")
        if tag == "(b)":
            verdict = ratio
        del off, on, legs
    lines.append(f"default rule: ReshapeClassBranch(fused=True) stays the default only if (b) shows on / off <= 1.00 in this run: "
                 f"{verdict:.2f} -> {'fused=True stays' if verdict <= 1.0 else 'fused must default to False'}; DenseClassBranch's "
                 f"default (fused_pool=False) does not depend on (c)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
