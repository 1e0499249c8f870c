"""CPU: the fused Adam's C ABI (scn_adam_many and its queries) and the host layer of sparse_rcnn_amd.optim.Adam --
constructor validation, refused options and devices, torch's state_dict layout.  No GPU: nothing is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_adam_and_binding_lists_it():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scn_mi355x.h")).read(), flags=re.S)
    fns = set(re.findall(r"\b(scn_[a-z0-9_]+)\s*\(", text))
    from sparse_rcnn_amd import _lib
    for name in ("scn_adam_many", "scn_adam_launches", "scn_adam_segment_bytes"):
        assert name in fns and name in _lib.EXPORTS
    text = open(os.path.join(ROOT, "include", "scn_mi355x.h")).read()
    assert "typedef struct scn_adam_segment" in text and "#define SCN_ABI_VERSION 5" in text


def _lib_loaded():
    import __graft_entry__
    __graft_entry__.build()
    from sparse_rcnn_amd import _lib
    return _lib.load()


def test_segment_layout_matches_the_binding():
    from sparse_rcnn_amd import optim
    lib = _lib_loaded()
    assert lib.scn_abi_version() == 5
    assert lib.scn_adam_segment_bytes() == optim.SEGMENT.itemsize == 56


def _table(n_segs, n=3):
    from sparse_rcnn_amd import optim
    t = np.zeros(n_segs, dtype=optim.SEGMENT)
    t["n"] = n
    t["p"], t["g"], t["m"], t["v"] = 1 << 12, 2 << 12, 3 << 12, 4 << 12       # never dereferenced: only counted
    t["step_size"], t["inv_bc2_sqrt"], t["decay"] = 1e-3, 30.0, 1.0
    return t


def test_launch_count_batches_segments_and_constant_sets():
    from sparse_rcnn_amd import optim
    _lib_loaded()
    assert optim.launches(_table(0)) == 0
    assert optim.launches(_table(80)) == 1
    assert optim.launches(_table(156)) == 2          # 80 segments per launch
    t = _table(10)
    t["step_size"] = np.arange(10) + 1.0             # ten constant sets, four per launch
    assert optim.launches(t) == 3
    t = _table(5)
    t["n"][:] = 0                                    # empty segments launch nothing
    assert optim.launches(t) == 0


@pytest.mark.parametrize("field,value", [("n", -1), ("p", 0), ("g", 0), ("m", 0), ("v", 0), ("p", (1 << 12) + 2),
                                         ("step_size", np.inf), ("inv_bc2_sqrt", np.nan), ("inv_bc2_sqrt", 0.0),
                                         ("weight_decay", np.inf), ("decay", np.nan)])
def test_bad_segment_is_einval(field, value):
    from sparse_rcnn_amd import _lib, optim
    lib = _lib_loaded()
    t = _table(4)
    t[field][2] = value
    n = ctypes.c_int(-1)
    assert lib.scn_adam_launches(t.ctypes.data, len(t), ctypes.byref(n)) == _lib.EINVAL
    assert b"segment 2" in lib.scn_last_error_string() or b"requirement" in lib.scn_last_error_string()
    # the launching entry point validates the whole table before anything is enqueued (so no GPU is touched here)
    assert lib.scn_adam_many(t.ctypes.data, len(t), 1.0, 0.9, 0.999, 1e-8, None) == _lib.EINVAL
    with pytest.raises(_lib.ScnError):
        optim.launches(t)


def test_null_pointer_with_zero_length_is_fine_and_null_table_is_einval():
    from sparse_rcnn_amd import _lib
    lib = _lib_loaded()
    t = _table(2)
    t["n"][1] = 0
    t["p"][1] = t["g"][1] = t["m"][1] = t["v"][1] = 0
    n = ctypes.c_int(-1)
    assert lib.scn_adam_launches(t.ctypes.data, 2, ctypes.byref(n)) == 0 and n.value == 1
    assert lib.scn_adam_launches(None, 3, ctypes.byref(n)) == _lib.EINVAL
    assert lib.scn_adam_launches(t.ctypes.data, -1, ctypes.byref(n)) == _lib.EINVAL


@pytest.mark.parametrize("args", [(np.nan, 0.999, 1e-8, 1.0), (0.9, np.inf, 1e-8, 1.0), (0.9, 0.999, np.nan, 1.0),
                                  (0.9, 0.999, 1e-8, np.inf)])
def test_non_finite_launch_arguments_are_einval(args):
    from sparse_rcnn_amd import _lib
    lib = _lib_loaded()
    b1, b2, eps, gs = args
    t = _table(3)
    assert lib.scn_adam_many(t.ctypes.data, 3, gs, b1, b2, eps, None) == _lib.EINVAL


def _p(shape=(3,), device="cpu"):
    return torch.nn.Parameter(torch.zeros(shape, device=device))


def test_constructor_validation_matches_torch():
    from sparse_rcnn_amd.optim import Adam
    p = [_p()]
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            torch.optim.Adam(p, **kw)
        with pytest.raises(ValueError):
            Adam(p, **kw)


@pytest.mark.parametrize("opt", ["amsgrad", "maximize", "capturable", "differentiable"])
def test_unsupported_options_raise(opt):
    from sparse_rcnn_amd.optim import Adam
    with pytest.raises(ValueError, match=opt):
        Adam([_p()], **{opt: True})


def test_cpu_parameters_are_refused():
    from sparse_rcnn_amd.optim import Adam
    with pytest.raises(ValueError, match="no CPU fallback"):
        Adam([_p()])
    with pytest.raises(ValueError, match="no CPU fallback"):
        Adam([{"params": [_p()], "lr": 1e-3}, {"params": [_p((2, 2))]}])


def test_fresh_state_dict_matches_torch_key_for_key(monkeypatch):
    """The reference's three groups (run.py:1441-1449).  The device check is lifted for this CPU-only layout comparison:
    a fresh optimizer has no state, so nothing is laid out or launched."""
    from sparse_rcnn_amd import optim
    monkeypatch.setattr(optim, "_check_param", lambda p: None)
    groups = lambda: [{"params": [_p(), _p((4, 2))]}, {"params": [_p((5,))]}, {"params": [_p((1,))], "lr": 1e-3}]  # noqa: E731
    kw = dict(lr=4e-4, weight_decay=0)
    ours = optim.Adam(groups(), **kw).state_dict()
    ref = torch.optim.Adam(groups(), **kw).state_dict()
    assert ours.keys() == ref.keys()
    assert ours["state"] == ref["state"] == {}
    assert len(ours["param_groups"]) == len(ref["param_groups"]) == 3
    for a, b in zip(ours["param_groups"], ref["param_groups"]):
        assert list(a.keys()) == list(b.keys())
        assert a == b
    o = optim.Adam(groups(), **kw)
    sched = torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.992)
    assert [g["lr"] for g in o.param_groups] == [4e-4, 4e-4, 1e-3]
    assert sched.get_last_lr() == [4e-4, 4e-4, 1e-3]


def test_sceneStep_rejects_unknown_optimizer():
    from sparse_rcnn_amd.trainstep import SceneStep
    with pytest.raises(ValueError, match="optimizer"):
        SceneStep("cfg2", device=torch.device("cpu"), optimizer="rmsprop")
