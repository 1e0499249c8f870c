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

from sparse_rcnn_amd import _lib as L
from sparse_rcnn_amd.trainstep import SceneStep

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
WARMUP = int(sys.argv[2]) if len(sys.argv) > 2 else 10
NAMES = {1: "gemm_ident", 2: "conv_subm", 3: "conv_child", 4: "rules_child", 5: "rows2", 6: "wgrad_subm", 7: "wgrad2_subm",
         8: "wgrad_down", 9: "wgrad_up", 10: "wgrad_ident", 11: "colsum", 12: "add", 13: "cast", 14: "relu", 15: "relu_bwd",
         16: "add_relu", 17: "bn_stats", 18: "bn_fwd", 19: "bn_bwd"}
QUIET = ("bytes", "counters", "version", "debug", "timing", "last_error", "step_begin", "step_hold", "step_flush",
         "step_discard", "group_counts", "requirements", "describe", "launches")


class _Counting:
    """The library handle with every launching entry point counted by name."""

    def __init__(self, lib):
        self._lib, self.calls, self._made = lib, collections.Counter(), {}

    def __getattr__(self, name):
        fn = self._made.get(name)
        if fn is None:
            raw = getattr(self._lib, name)
            if any(q in name for q in QUIET):
                fn = raw
            else:
                def fn(*a, _raw=raw, _name=name):
                    self.calls[_name] += 1
                    return _raw(*a)
            self._made[name] = fn
        return fn


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
    counting = _Counting(lib)
    L._lib = counting
    lib.scn_exec_timing_enable(2)
    try:
        job.step()
        torch.cuda.synchronize()
    finally:
        lib.scn_exec_timing_enable(0)
        L._lib = lib
    cap = 16384
    tms, info = (C.c_float * cap)(), (C.c_int64 * (7 * cap))()
    ops = lib.scn_exec_timing_collect(tms, info, cap)
    by_op = collections.Counter()                  # us inside the executor's ops of the counted step, per op kind
    for k in range(ops):
        by_op[NAMES.get(int(info[7 * k]), int(info[7 * k]))] += float(tms[k]) * 1e3
    runs = sum(v for k, v in counting.calls.items() if k.startswith("scn_exec_run"))
    calls = sum(counting.calls.values()) - runs + ops
    nodes = _nodes(job.out.features)
    what = job.describe()
    job.finish()
    return dict(ms=ms, calls=calls, exec_runs=runs, exec_ops=ops, nodes=sum(nodes.values()),
                stage_nodes=sum(v for k, v in nodes.items() if k.startswith("StageFunction")),
                bn_nodes=sum(v for k, v in nodes.items() if k.startswith("BatchNormReLUFunction")),
                groups=list(groups), what=what, by_op=by_op, py_calls=counting.calls)


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
