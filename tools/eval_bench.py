"""Times the evaluation on the device against the dense-mask formulation it replaces, run in torch on the same GPU, and
SceneStep.evaluate (its output is what a profiles/eval.txt would hold).  Device events around back-to-back calls through the Python API (host launch cost
included); the minimum of three runs.

    python tools/eval_bench.py [--reps 20] [--skip-step] [--bench-ab PARENT_CHECKOUT]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = torch.device("cuda", 0)


def timed(fn, reps, runs=3):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return min(out), out


def torch_mask_iou(pred, gt, rows_per_pass=32):
    """The formulation the device path replaces, in torch on the same GPU: bool masks, 32 predictions per pass, every pass
    materialises the [32, G, N] intersection and union, converts both to fp32 and sums over the points."""
    parts = []
    for start in range(0, pred.shape[0], rows_per_pass):
        rows = pred[start:start + rows_per_pass, None, :]
        both, either = rows & gt[None], rows | gt[None]
        parts.append(both.float().sum(-1) / either.float().sum(-1))
    return torch.cat(parts) if parts else pred.new_zeros((0, gt.shape[0]), dtype=torch.float32)


def torch_greedy_match(iou, threshold):
    """Greedy matching as a host loop over device tensors, one host wait per prediction (the formulation scn_eval_match
    replaces): every prediction in turn takes the best ground truth that is still free, if it reaches the threshold."""
    free = torch.ones(iou.shape[1], dtype=torch.bool, device=iou.device)
    hit = torch.zeros(iou.shape[0], dtype=torch.bool, device=iou.device)
    for i in range(iou.shape[0]):
        cand = torch.nonzero(free).squeeze(1)
        if cand.numel() == 0:
            break
        vals = iou[i, cand]
        j = int(vals.argmax())
        if bool(vals[j] >= threshold):
            free[cand[j]] = False
            hit[i] = True
    return hit


def shape_case(b, p, g, n, reps, k=18):
    from sparse_rcnn_amd import evaluation as E, roi
    from sparse_rcnn_amd.loss import pack_gt_masks
    gen = torch.Generator(device=DEV).manual_seed(p + g + n)
    gt = [torch.rand((g, n), device=DEV, generator=gen) < torch.empty((g, 1), device=DEV).uniform_(0.001, 0.3, generator=gen)
          for _ in range(b)]
    # a selection: every box takes ~10 % of its sample's points; half of the boxes sit on a ground truth
    inside = torch.zeros((b * p, b * n), dtype=torch.bool, device=DEV)
    for s in range(b):
        blk = torch.rand((p, n), device=DEV, generator=gen) < 0.1
        blk[::2] |= gt[s][torch.arange(0, p, 2, device=DEV) % g]
        inside[s * p:(s + 1) * p, s * n:(s + 1) * n] = blk
    nz = inside.nonzero()
    prefix = [0] + torch.cumsum(inside.sum(1), 0).tolist()
    sel = roi.RoiSelection(nz[:, 1].to(torch.int32).contiguous(), nz[:, 0].to(torch.int32).contiguous(), prefix, b * n, b * p)
    del inside, nz
    m = sel.src_row.shape[0]
    logits = torch.randn((m, k), device=DEV, generator=gen) * 2
    cls = torch.randint(0, k, (b * p,), device=DEV, generator=gen)
    counts, splits = [p] * b, [n] * b
    gt_packed = pack_gt_masks(gt)
    score = [torch.rand(p, device=DEV, generator=gen).sort(descending=True)[0] for _ in range(b)]
    pcls = list(cls.split(p))
    gcls = [c[torch.arange(g, device=DEV) % p] for c in pcls]
    thresholds, classes = [0.25, 0.5], list(range(k))

    state = {}

    def device_iou():
        state["r"] = E.mask_iou(E.mask_bits(logits, sel, counts, splits, cls), gt_packed)

    def torch_iou():
        masks = roi.mask_predict(logits, sel, counts, splits, cls)
        state["t"] = [torch_mask_iou(mk > 0.5, gs) for mk, gs in zip(masks, gt)]

    def device_iou_only():
        E.mask_iou(state["bits"], gt_packed)

    dev_ms, dev_runs = timed(device_iou, reps)
    ref_ms, ref_runs = timed(torch_iou, max(reps // 10, 2))
    for s in range(b):
        want, got = state["t"][s], state["r"].sample(s)["iou"]
        assert torch.equal(torch.isnan(want), torch.isnan(got)) and torch.equal(torch.nan_to_num(want), torch.nan_to_num(got))
    state["bits"] = E.mask_bits(logits, sel, counts, splits, cls)
    iou_ms, _ = timed(device_iou_only, reps)
    w = (n + 31) // 32
    tiles = b * -(-p // 64) * -(-g // 64)
    tile_bytes = tiles * 128 * w * 4                                      # packed inputs read once per tile pass
    ious = [state["r"].sample(s)["iou"] for s in range(b)]
    keep = [sc >= 0.2 for sc in score]

    def device_match():
        state["f"] = E.match(ious, thresholds, keep, pcls, gcls, classes)[0]

    def torch_match():
        out = []
        for c in [None] + classes:
            for t in thresholds:
                for s in range(b):
                    kp = keep[s] if c is None else keep[s] & (pcls[s] == c)
                    cols = slice(None) if c is None else (gcls[s] == c)
                    out.append(torch_greedy_match(ious[s][kp][:, cols], t))
        state["m"] = out

    match_ms, match_runs = timed(device_match, reps)
    t0 = time.perf_counter()
    torch_match()
    torch.cuda.synchronize()
    ref_match_ms = (time.perf_counter() - t0) * 1e3
    f, i = state["f"].cpu(), 0
    for ci in range(1 + k):
        for ti in range(2):
            o = 0
            for s in range(b):
                got = f[ci, ti, o:o + p]
                assert torch.equal(got[got >= 0] > 0, state["m"][i].cpu()), (ci, ti, s)
                o += p
                i += 1
    n_tp = int((f > 0).sum())
    name = f"{b} x ({p}, {g}, {n})"
    print(f"mask IoU {name}: device (scn_eval_mask_bits + scn_eval_mask_iou, {m} selected rows) {dev_ms:.4f} ms (runs "
          f"{' '.join(f'{x:.4f}' for x in dev_runs)}), torch (mask_predict -> > 0.5 -> [32, G, N] broadcast) {ref_ms:.3f} ms (runs "
          f"{' '.join(f'{x:.3f}' for x in ref_runs)}), torch / device {ref_ms / dev_ms:.1f}x; scn_eval_mask_iou alone {iou_ms:.4f} ms "
          f"= {tile_bytes / iou_ms / 1e6:.1f} GB/s of its {tile_bytes / 1e6:.1f} MB algorithmic bytes ({tiles} tiles of 64 x 64, "
          f"host launch cost of 4 calls included); IoU matrices bit-equal", flush=True)
    print(f"matching {name}: {(1 + k) * 2 * b} problems ({n_tp} true positives): scn_eval_match {match_ms:.4f} ms (runs "
          f"{' '.join(f'{x:.4f}' for x in match_runs)}), a Python loop on device tensors (one host wait per prediction) {ref_match_ms:.1f} ms (one "
          f"run), loop / device {ref_match_ms / match_ms:.0f}x; flags equal", flush=True)
    return ref_ms >= dev_ms and ref_match_ms >= match_ms


def step_case(workload, **kw):
    from sparse_rcnn_amd.trainstep import SceneStep
    from sparse_rcnn_amd import evaluation as E
    st = SceneStep(workload, optimizer="adam", rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True,
                   prefetch=False, lr=1e-4, **kw)
    for _ in range(3):
        st.step()
    st.finish()
    st.evaluate(score_threshold=0.0)
    st.finish()
    t = float(torch.cat([r["score"] for r in st.eval_out["overlap"]["bbox"].records]).median().item())
    total, metrics = [], []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.evaluate(score_threshold=t)
        torch.cuda.synchronize()
        total.append((time.perf_counter() - t0) * 1e3)
        st.finish()
        out = st.eval_out
        for a in out["overlap"].values():
            a._cache = {}
        helper = E.EvaluationHelper([0.25, 0.5], list(range(18)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        helper(out["overlap"], {"segment": out["segment"]}, {"gtbbox": out["gtbbox"]}, {"gtlabelmask": out["gtlabelmask"]})
        torch.cuda.synchronize()
        metrics.append((time.perf_counter() - t0) * 1e3)
    n_scenes = st.batches_per_step
    boxes = sum(int(r["score"].shape[0]) for r in out["overlap"]["bbox"].records)
    print(f"SceneStep.evaluate {workload} {kw}: {min(total):.2f} ms per call ({n_scenes} micro-batch, {len(out['overlap']['bbox'].records)} "
          f"sample(s), {boxes} proposals; wall clock, host waits included; runs {' '.join(f'{x:.2f}' for x in total)}); of that the "
          f"metrics (EvaluationHelper: 5 matching launches, 7 host waits, curves) {min(metrics):.2f} ms, forward + overlaps "
          f"{min(total) - min(metrics):.2f} ms", flush=True)


def bench_ab(parent_dir, rounds=3):
    """`bench.py --workload cfg3-rpn` in a built checkout of the parent commit and in this tree, alternating, each run a
    fresh process: the default step runs no new code and must stay inside the parent's spread."""
    import json
    import subprocess
    print("# python bench.py --gpus 1 --steps 50 --warmup 10 --workload cfg3-rpn, the parent commit's tree and this one alternating:",
          flush=True)
    for i in range(1, rounds + 1):
        for side, cwd in (("parent", parent_dir), ("change", ROOT)):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10", "--workload", "cfg3-rpn"],
                               cwd=cwd, capture_output=True, text=True, timeout=150)
            if r.returncode != 0:
                raise SystemExit(f"bench.py failed in {cwd} ({r.returncode}): {r.stderr[-400:]}")
            d = json.loads(r.stdout.strip().splitlines()[-1])
            print(f"{side} {i}: ms_per_step {d.get('ms_per_step')} value {d.get('value')}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--bench-ab", metavar="PARENT_DIR", help="a built checkout of the parent commit: alternate bench.py runs")
    args = ap.parse_args()
    print(f"# evaluation on the device vs the reference's formulation in torch on the same GPU ({torch.cuda.get_device_name(0)}); "
          f"ms per call, device events around back-to-back calls through the Python API", flush=True)
    ok = True
    for shape in ((1, 64, 64, 172_500), (1, 256, 64, 172_500), (12, 256, 256, 14_375)):
        ok &= shape_case(*shape, reps=args.reps)
    print(f"# requirement 'not slower at any of the three shapes': {'met' if ok else 'MISSED'}", flush=True)
    if not args.skip_step:
        step_case("cfg3-rpn")
        step_case("ref-crop-rpn", n_gt=8)
    if args.bench_ab:
        bench_ab(os.path.abspath(args.bench_ab))


if __name__ == "__main__":
    main()
