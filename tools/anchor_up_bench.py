"""Device time of the up-sampling RPN heads at the reference's shape -- 12 crops of 128 x 128 x 64 voxels, anchor levels
32 x 32 x 16 x 128 (stride 4) and 16 x 16 x 8 x 256 (stride 8), 11 groups, 182 272 anchors per crop of which 88 536 lie inside:

  1. the two new calls (scn_anchor_up_fwd / _bwd behind functional.AnchorUpFunction) against the restatement run as torch
     operators on the same device tensors (tests/anchor_up_restate.py: per group view / permute / reshape, cat, mask, split),
     and the bytes they move over their time;
  2. the whole head (row GEMM + scatter, rpn.AnchorNetworkUpsample) forward and backward;
  3. SceneStep('ref-crop-rpn', rpn_loss=True) with upsample_heads False and True, alternating;
  4. with --parent DIR (a built checkout of the parent commit): `bench.py --workload ref-crop-rpn` there and here, alternating.

Medians of alternating rounds, inputs resident.

    python tools/anchor_up_bench.py [--out profiles/anchor_up.txt] [--parent DIR] [--skip-steps]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_ACHIEVABLE = 6.3e12            # MI355X: bytes/s a streaming kernel reaches


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


def rounds_line(name, v):
    return f"{name}: median {statistics.median(v):.4f} ms (rounds {' '.join(f'{x:.4f}' for x in v)})"


def kernels_and_head(lines, n_rounds):
    import anchor_up_restate as A
    from sparse_rcnn_amd import rpn as R
    from sparse_rcnn_amd.functional import AnchorUpFunction
    dev = torch.device("cuda")
    batch, scene = 12, (128, 128, 64)
    torch.manual_seed(0)
    net = R.AnchorNetworkUpsample(R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS, (4, 8), (128, 256),
                                  extra_stride_levels=R.REF_EXTRA_STRIDE_LEVELS).to(dev)
    sizes = net.level_sizes(scene)
    pl = net.plan(scene, sizes, dev)
    groups = [[(g["extra"], g["n_anchors"]) for g in lv] for lv in net._groups]
    inside = pl.inside_cpu.to(dev)
    g = torch.Generator().manual_seed(0)
    Ps = [torch.randn((batch * s[0] * s[1] * s[2], n), generator=g).to(dev).requires_grad_() for s, n in zip(sizes, net.ncol_levels)]
    d_bbox = torch.randn((batch, pl.n_inside, 2, 3), generator=g).to(dev)
    d_score = torch.randn((batch, pl.n_inside), generator=g).to(dev)
    p_bytes = sum(P.numel() for P in Ps) * 4
    rec_bytes = batch * pl.n_inside * 28
    lines.append(f"shape: {batch} crops of {scene[0]}x{scene[1]}x{scene[2]}; P {' + '.join(f'{tuple(P.shape)}' for P in Ps)} fp32 = "
                 f"{p_bytes / 1e6:.1f} MB; {pl.n_all} anchors per crop, {pl.n_inside} inside; outputs {rec_bytes / 1e6:.1f} MB")

    def ours_fwd():
        return AnchorUpFunction.apply(pl, batch, *Ps)

    out = ours_fwd()

    def ours_bwd():
        for P in Ps:
            P.grad = None
        torch.autograd.backward(list(out), [d_bbox, d_score], retain_graph=True)

    def ref_fwd():
        return A.permute_restated(Ps, batch, sizes, groups, inside)

    def ref_both():
        for P in Ps:
            P.grad = None
        torch.autograd.backward(list(ref_fwd()), [d_bbox, d_score])

    rb, rs = ref_fwd()
    lines.append(f"ours vs restatement: rpn_bbox bit-equal {torch.equal(out[0], rb)}, rpn_score bit-equal {torch.equal(out[1], rs)}")
    t = {"scn_anchor_up_fwd (both levels)": [], "restated fwd": [], "scn_anchor_up_bwd (both levels)": [], "restated fwd + bwd": []}
    for _ in range(n_rounds):                                   # alternating
        t["scn_anchor_up_fwd (both levels)"].append(timed(ours_fwd, 20))
        t["restated fwd"].append(timed(ref_fwd, 5, 1))
        t["scn_anchor_up_bwd (both levels)"].append(timed(ours_bwd, 20))
        t["restated fwd + bwd"].append(timed(ref_both, 5, 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    for k, v in t.items():
        lines.append(rounds_line(k, v))
    fwd, bwd = med["scn_anchor_up_fwd (both levels)"], med["scn_anchor_up_bwd (both levels)"]
    # the forward reads P only where dest >= 0 (the records of the inside anchors) and all of dest; the backward writes all of dP
    for name, ms, moved, what in (("scn_anchor_up_fwd", fwd, 2 * rec_bytes + pl.n_all * 4,
                                   "the inside anchors' elements of P read + records written once + dest; 4-byte accesses"),
                                  ("scn_anchor_up_bwd", bwd, p_bytes + rec_bytes + pl.n_all * 4,
                                   "dP written once + records read once + dest")):
        lines.append(f"{name}: {moved / 1e6:.1f} MB ({what}) in {ms:.4f} ms = {moved / ms / 1e9:.2f} TB/s = "
                     f"{100 * moved / ms / 1e-3 / HBM_ACHIEVABLE:.0f} % of the 6.3 TB/s a streaming kernel reaches")
    lines.append(f"kernels fwd + bwd {fwd + bwd:.4f} ms against the restatement's {med['restated fwd + bwd']:.4f} ms "
                 f"({med['restated fwd + bwd'] / (fwd + bwd):.1f} x)")
    del out, rb, rs

    # ---- the whole head: row GEMM + scatter ----
    slabs = [torch.randn((batch * s[0] * s[1] * s[2], c), generator=g).to(dev).requires_grad_() for s, c in zip(sizes, (128, 256))]
    args = [(x, s, batch) for x, s in zip(slabs, sizes)]

    def head_fwd():
        with torch.no_grad():
            return net(args, scene)

    def head_both():
        for x in slabs:
            x.grad = None
        for p in net.parameters():
            p.grad = None
        bbox, score, _ = net(args, scene)
        torch.autograd.backward([bbox, score], [d_bbox, d_score])

    tf, tb = [], []
    for _ in range(n_rounds):
        tf.append(timed(head_fwd, 10))
        tb.append(timed(head_both, 10))
    lines.append(rounds_line("whole head forward (pack + 2 row GEMMs + 2 scatters)", tf))
    lines.append(rounds_line("whole head forward + backward (to the slabs, the 22 parameters)", tb))


def steps(lines, n_rounds=3, n_steps=10):
    from sparse_rcnn_amd.trainstep import SceneStep
    jobs = {False: SceneStep("ref-crop-rpn", rpn_loss=True), True: SceneStep("ref-crop-rpn", rpn_loss=True, upsample_heads=True)}
    import time
    t = {False: [], True: []}
    for up, job in jobs.items():
        for _ in range(3):
            job.step()
        job.finish()
    for _ in range(n_rounds):                                   # alternating
        for up, job in jobs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                job.step()
            job.finish()
            torch.cuda.synchronize()
            t[up].append((time.perf_counter() - t0) * 1e3 / n_steps)
    for up in (False, True):
        n = jobs[up]._rpn_target_setup(0)[0].anchors.shape[0]
        lines.append(rounds_line(f"SceneStep('ref-crop-rpn', rpn_loss=True, upsample_heads={up}) ms/step, {n} inside anchors per crop", t[up]))
    a, b = statistics.median(t[False]), statistics.median(t[True])
    lines.append(f"the reference's heads and anchor set cost {b - a:+.3f} ms per step ({100 * (b - a) / a:+.1f} %): head, targets, draw, "
                 "loss and top-k on 88 536 instead of 36 240 inside anchors per crop")


def bench_pair(lines, parent, n_rounds=3, n_steps=20, warmup=5):
    def run(tree):
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(n_steps), "--warmup", str(warmup),
                            "--workload", "ref-crop-rpn"], cwd=tree, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"bench.py failed in {tree}: {r.stderr[-2000:]}")
        doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        return doc
    t = {"parent": [], "this change": []}
    key = "ms_per_step"
    for _ in range(n_rounds):                                   # alternating
        for name, tree in (("parent", parent), ("this change", ROOT)):
            t[name].append(float(run(tree)[key]))
    for name, v in t.items():
        lines.append(f"bench.py --workload ref-crop-rpn, {name}: {key} {' '.join(f'{x:.4f}' for x in v)} (median {statistics.median(v):.4f})")
    lo, hi = min(t["parent"]), max(t["parent"])
    inside = all(lo <= x <= hi for x in t["this change"])
    lines.append(f"the default runs of this change lie {'inside' if inside else 'NOT all inside'} the parent's spread [{lo:.4f}, {hi:.4f}]")


class Lines(list):
    """The report, printed as it grows (a run cut short keeps what it measured)."""

    def append(self, line):
        print(line, flush=True)
        super().append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py there and here, alternating")
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    lines = Lines()
    kernels_and_head(lines, args.rounds)
    if not args.skip_steps:
        steps(lines)
        torch.cuda.empty_cache()
    if args.parent:
        torch.cuda.empty_cache()
        bench_pair(lines, args.parent)
    else:
        lines.append("bench.py parent against this change: NOT MEASURED in this run (no --parent tree given)")
    text = "\n".join(lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
