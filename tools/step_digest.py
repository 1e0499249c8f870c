"""What `trainstep.SceneStep` computes, case by case, as digests: the tool two commits are compared with after a change that must
not move a bit.  One process, the cases one after another, each at the small shapes the GPU tests use.

    python tools/step_digest.py --out A.json [--cases SUBSTRING ...]
    python tools/step_digest.py --compare A.json B.json        # prints every key that differs; exit status 1 if any does

Per case: the step is built, runs two `step()` calls and `finish()`; `forward_only(0)` where it has no losses; `predict(0)` and
`evaluate(score_threshold=0.5)` where it has the class branch; and, last, one more step with the library's launching calls
counted (tools/call_count.py).  Recorded: a SHA-256 of the flat parameters before and after the two steps, of `out.features`,
`fin.grad`, `logits`, every `*_losses` value and `loss_record`, of the forward_only and predict outputs and `predict_out`; the
evaluate metric dicts; the `describe()` text; the launching calls of a step.

The cases are those of tests/golden/make_step_wiring_golden.py (the steps that can also be constructed without a GPU) and the
ones that cannot: the four-loss step in f32 and bf16, with Adam, with accumulation and learned loss weights, as the mask-only
stage initialised from an earlier one; `step_group=False`; `weighting="count"` on one rank."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch

import make_step_wiring_golden as G
from call_count import counted, launching_calls

FOUR = dict(rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True)
SMALL = dict(target=10_000, grid=(128, 128, 64))
SHAPES = {"cfg3-rpn": dict(SMALL, n_gt=4), "ref-crop-rpn": dict(grid=(64, 32, 32), target=3000, n_gt=4)}
# behind the 1x1 heads the selector's top-1024 over the inside anchors of a 64 x 32 x 32 crop is refused (k out of range, on any
# commit): that one case runs on the workload's own grid
CASE_SHAPES = {"ref-crop-rpn/bare": dict(grid=(128, 128, 64), target=3000, n_gt=4)}


def all_cases():
    """name -> (workload, keywords beyond the shape)."""
    cases = dict(G.case_keywords())
    cases.update({
        "cfg3-rpn/four/f32": ("cfg3-rpn", dict(FOUR)),
        "cfg3-rpn/four/bf16": ("cfg3-rpn", dict(FOUR, dtype="bf16")),
        "cfg3-rpn/four/adam": ("cfg3-rpn", dict(FOUR, optimizer="adam")),
        "cfg3-rpn/four/batches_per_step2-multitask": ("cfg3-rpn", dict(FOUR, batches_per_step=2, multitask_loss=True)),
        "cfg3-rpn/four/train=mask-init_state": ("cfg3-rpn", dict(FOUR, train=("mask",), init_state=G.EARLIER_STAGE)),
        "cfg2/step_group=False": ("cfg2", dict(step_group=False)),
        "cfg2/weighting=count": ("cfg2", dict(weighting="count")),
    })
    return cases


def sha(value):
    """A tensor's bytes, None, a crop selection, or a (nested) sequence / mapping of those -> one SHA-256 (None for None)."""
    if value is None:
        return None
    h = hashlib.sha256()

    def feed(v):
        if v is None:
            h.update(b"<none>")
        elif torch.is_tensor(v):
            t = v.detach().to("cpu").contiguous()
            h.update(f"{t.dtype}{tuple(t.shape)}".encode())
            h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
        elif isinstance(v, dict):
            for k in v:
                h.update(str(k).encode())
                feed(v[k])
        elif isinstance(v, (list, tuple)):
            h.update(f"<{len(v)}>".encode())
            for x in v:
                feed(x)
        elif hasattr(v, "src_row"):                              # roi.RoiSelection: the crop's list form
            feed([v.src_row, v.box_of, v.prefix, v.n_points, v.n_boxes, v.new_coords])
        else:
            h.update(repr(v).encode())
    feed(value)
    return h.hexdigest()


def plain(v):
    """A metric dict as JSON holds it: keys as strings, numbers as their `repr` (a NaN then equals a NaN)."""
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if torch.is_tensor(v):
        return plain(v.tolist())
    return v if isinstance(v, (str, bool, type(None))) else repr(float(v))


def run_case(name, workload, keywords):
    shape = dict(device=torch.device("cuda", 0), **CASE_SHAPES.get(name, SHAPES.get(workload, SMALL)))
    step = G.build(workload, keywords, shape)
    rec = {"describe_built": step.describe(), "flat_initial": sha(step.flat.flat)}
    step.step()
    step.step()
    step.finish()
    torch.cuda.synchronize()
    rec["flat_after"] = sha(step.flat.flat)
    rec["out.features"], rec["fin.grad"], rec["logits"] = sha(step.out.features), sha(step.fin.grad), sha(step.logits)
    for key in ("rpn_losses", "mask_losses", "class_losses", "segmentation_losses"):
        rec[key] = sha(getattr(step, key))
    rec["loss_record"] = None if step.loss_record is None else [list(step.loss_record), sha(step.loss_record.tensor)]
    rec["describe"] = step.describe()
    has_losses = step.rpn_loss or step.mask_loss or step.class_loss or step.segmentation_loss
    if not has_losses:
        out, logits = step.forward_only(0)
        step.finish()
        rec["forward_only"] = [sha(out.features), sha(logits)]
    if step.model.class_branch is not None:
        rec["predict"] = sha(step.predict(0))
        step.finish()
        class_scores, logits, (sel, counts, splits) = step.predict_out
        rec.update({"predict_out.class_scores": sha(class_scores), "predict_out.logits": sha(logits),
                    "predict_out.selection": sha(sel), "predict_out.counts": sha(counts), "predict_out.splits": sha(splits)})
        combined, single_class = step.evaluate(score_threshold=0.5)
        rec["evaluate"] = [plain(combined), plain(single_class)]
    calls, ops = counted(step.step)
    step.finish()
    rec["launching_calls"] = list(launching_calls(calls, ops)) + [dict(sorted(calls.items()))]
    return rec


def compare(a_path, b_path):
    with open(a_path) as f:
        a = json.load(f)
    with open(b_path) as f:
        b = json.load(f)
    differ = 0
    for case in sorted(set(a) | set(b)):
        ra, rb = a.get(case), b.get(case)
        if ra is None or rb is None:
            print(f"{case}: only in {b_path if ra is None else a_path}")
            differ += 1
            continue
        for key in sorted(set(ra) | set(rb)):
            if ra.get(key) != rb.get(key):
                print(f"{case}: {key} differs\n    {json.dumps(ra.get(key))[:300]}\n    {json.dumps(rb.get(key))[:300]}")
                differ += 1
    print(f"{len(set(a) | set(b))} cases, {differ} differing keys")
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", nargs="+", default=None, help="run only the cases whose name contains one of these")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"), default=None)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    cases = {n: c for n, c in all_cases().items() if args.cases is None or any(s in n for s in args.cases)}
    if not torch.cuda.is_available():
        print("no GPU: nothing run; the cases are\n  " + "\n  ".join(cases))
        return
    if not args.out:
        ap.error("--out required")
    results = {}
    for name, (workload, keywords) in cases.items():
        results[name] = run_case(name, workload, keywords)
        print(f"{name}: done", flush=True)
        with open(args.out, "w") as f:                       # (rewritten after every case: a run that ends early leaves what it had)
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
