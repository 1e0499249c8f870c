"""cfg2-bn as step-executor stages against the layer-by-layer path, in ONE process: library calls that launch kernels,
autograd nodes and event-timed milliseconds per step (forward + backward + update, `SceneStep.step`).
    python tools/bn_stages_bench.py [steps] [warmup]

"launching calls": entry points of the library that queue kernels.  Layer by layer every one is a ctypes call from Python; in a
staged step the calls made from Python are counted the same way and every `scn_exec_run*` counts as the ops of its plan
(scn_exec_timing_enable(2) records one entry per op).  An entry point is one to three kernel launches on either path (scn_bn_stats
2, scn_bn_bwd 3, a weight gradient its units + its sum); in a staged backward the weight gradients' units and sums run as
grouped launches per pass -- `scn_wgrad_group_counts` gives those."""
import collections
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from call_count import counted, launching_calls
from sparse_rcnn_amd import _lib as L
from sparse_rcnn_amd.trainstep import SceneStep

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 10
NAMES = {1: "gemm_ident", 2: "conv_subm", 3: "conv_child", 4: "rules_child", 5: "rows2", 6: "wgrad_subm", 7: "wgrad2_subm",
         8: "wgrad_down", 9: "wgrad_up", 10: "wgrad_ident", 11: "colsum", 12: "add", 13: "cast", 14: "relu", 15: "relu_bwd",
         16: "add_relu", 17: "bn_stats", 18: "bn_fwd", 19: "bn_bwd", 20: "grad_norm", 21: "grad_scale"}

def _nodes(t):
    names, seen, todo = collections.Counter(), set(), [t.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names[type(f).__name__] += 1
        todo += [g for g, _ in f.next_functions]
    return names


def measure(**kw):
    job = SceneStep("cfg2-bn", torch.device("cuda", 0), **kw)
    for _ in range(WARMUP):
        job.step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        job.step()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / STEPS
    # one more step for the grouped weight-gradient launches it makes, then one with every call counted (neither is timed; the
    # per-op records of the second switch the grouping off)
    lib = L.lib()
    groups = (C.c_int64 * 4)()
    lib.scn_wgrad_group_counts(None, 1)
    job.step()
    torch.cuda.synchronize()
    lib.scn_wgrad_group_counts(groups, 1)
    py_calls, op_times = counted(job.step)
    by_op = collections.Counter()                  # us inside the executor's ops of the counted step, per op kind
    for op, ms_op in op_times:
        by_op[NAMES.get(op, op)] += ms_op * 1e3
    calls, runs, ops = launching_calls(py_calls, op_times)
    nodes = _nodes(job.out.features)
    what = job.describe()
    job.finish()
    return dict(ms=ms, calls=calls, exec_runs=runs, exec_ops=ops, nodes=sum(nodes.values()),
                stage_nodes=sum(v for k, v in nodes.items() if k.startswith("StageFunction")),
                bn_nodes=sum(v for k, v in nodes.items() if k.startswith("BatchNormReLUFunction")),
                groups=list(groups), what=what, by_op=by_op, py_calls=py_calls)


if __name__ == "__main__":
    rows = [("layer by layer", measure()), ("stages (bn_stages=True)", measure(bn_stages=True))]
    print(f"cfg2-bn, {STEPS} timed steps after {WARMUP} warm-up steps, one process")
    for name, r in rows:
        print(f"  {name:24s} {r['ms']:7.3f} ms/step  {r['calls']:4d} launching calls/step ({r['exec_runs']} executor passes holding "
              f"{r['exec_ops']} ops)  {r['nodes']:4d} autograd nodes ({r['stage_nodes']} StageFunction, {r['bn_nodes']} "
              f"BatchNormReLUFunction)  scn_wgrad_group_counts of a plain step: {r['groups']}")
    for name, r in rows:
        at = r["what"].find("BatchNormReLU")
        print(f"  {name}: describe() says \"" + r["what"][at:r["what"].find(")", at) + 1] + "\"")
        if r["by_op"]:
            print("    us per step inside the executor's ops (events around every op; grouping off while they are taken): "
                  + ", ".join(f"{k} {v:.0f}" for k, v in r["by_op"].most_common()) + f"; sum {sum(r['by_op'].values()):.0f}")
        else:
            print("    calls from Python: " + ", ".join(f"{k[4:]} {v}" for k, v in r["py_calls"].most_common(12)))
