"""Library calls that launch kernels, counted around a piece of Python: the wrapper tools/bn_stages_bench.py, tools/train_parts_bench.py
and tools/step_digest.py share.

"launching calls": entry points of the library that queue kernels.  Every one made from Python is a ctypes call through the
handle `_lib.lib()` returns, counted here by name; a `scn_exec_run*` call counts as the ops of its plan
(scn_exec_timing_enable(2) records one entry per op, which also switches the weight gradients' grouping off while it is on)."""
import collections
import ctypes as C

import torch

from sparse_rcnn_amd import _lib as L

QUIET = ("bytes", "counters", "version", "debug", "timing", "last_error", "step_begin", "step_hold", "step_flush",
         "step_discard", "group_counts", "requirements", "describe", "launches")


_INTS = (L.i32, L.i64, C.c_uint32, C.c_uint64)


def describe_call(name, args):
    """One call as text: every integer argument (by the argtypes of `_lib._SIGS`) as its value, every pointer argument as `p`,
    or `0` where it is NULL, every floating-point argument as `f`."""
    out = []
    for a, t in zip(args, L._SIGS[name][1]):
        if t in _INTS:
            out.append(str(int(getattr(a, "value", a))))
        elif t in (L.f32, C.c_double):
            out.append("f")
        else:
            v = getattr(a, "value", a) if isinstance(a, (C.c_void_p, C.c_char_p)) else a
            out.append("0" if v is None or (isinstance(v, int) and v == 0) or not bool(v) else "p")
    return f"{name}({','.join(out)})"


class _Counting:
    """The library handle with every launching entry point counted by name.  log: a list that receives `describe_call` of every
    counted call in order, and of the QUIET calls whose name starts with one of `log_also` (those stay uncounted)."""

    def __init__(self, lib, log=None, log_also=()):
        self._lib, self.calls, self._made = lib, collections.Counter(), {}
        self.log, self._log_also = log, tuple(log_also)

    def __getattr__(self, name):
        fn = self._made.get(name)
        if fn is None:
            raw = getattr(self._lib, name)
            quiet = any(q in name for q in QUIET)
            logged = self.log is not None and (not quiet or name.startswith(self._log_also))
            if quiet and not logged:
                fn = raw
            else:
                def fn(*a, _raw=raw, _name=name):
                    if not quiet:
                        self.calls[_name] += 1
                    if logged:
                        self.log.append(describe_call(_name, a))
                    return _raw(*a)
            self._made[name] = fn
        return fn


def counted(fn, cap=65536):
    """fn() with every call counted, the device idle when it returns.
    -> (calls from Python by name, [(op code, ms)] of the ops inside the `scn_exec_run*` calls among them)"""
    lib = L.lib()
    counting = _Counting(lib)
    L._lib = counting
    lib.scn_exec_timing_enable(2)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.scn_exec_timing_enable(0)
        L._lib = lib
    tms, info = (C.c_float * cap)(), (C.c_int64 * (7 * cap))()
    ops = lib.scn_exec_timing_collect(tms, info, cap)
    return counting.calls, [(int(info[7 * k]), float(tms[k])) for k in range(ops)]


def launching_calls(calls, ops):
    """(total launching calls, executor passes among them, ops inside those passes) of what `counted` returned."""
    runs = sum(v for k, v in calls.items() if k.startswith("scn_exec_run"))
    return sum(calls.values()) - runs + len(ops), runs, len(ops)
