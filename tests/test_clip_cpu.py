"""Global-norm gradient clipping without a GPU: the two executor ops are declared and bound consistently and add no entry point;
`scn_exec_requirements` counts the norm's partial sums and refuses a negative count; the float64 restatement the GPU tests compare
against (tests/clip_restate.py) agrees with torch.nn.utils.clip_grad_norm_; SceneStep(max_grad_norm=) constructs, describes the
clip, leaves the default description as it was and refuses bad bounds; optim.clip_grad_norm_ refuses what it does not implement."""
import ctypes as C
import hashlib
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # tests/clip_restate.py
import clip_restate as R                                                 # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = dict(device=torch.device("cpu"), channels=(16, 32), target=500, grid=(32, 32, 16), prefetch=False)
# sha256 of SceneStep("cfg2", **SMALL).describe() before the keyword existed (SGD: an Adam step did not construct on the CPU then)
DEFAULT_DESCRIBE_SHA256 = "a6f662c10848a53ca19450ecd5aaa7a5cde5b9577ef4408bb1a3c30bacba295b"


def _header():
    return open(os.path.join(HERE, "..", "include", "scn_mi355x.h")).read()


def test_the_ops_are_declared_and_bound_and_add_no_entry_point():
    from sparse_rcnn_amd import _lib as L, executor as EX
    header = _header()
    assert EX.OP_GRAD_NORM == 20 and EX.OP_GRAD_SCALE == 21
    assert re.search(r"SCN_OP_GRAD_NORM = 20\b", header) and re.search(r"SCN_OP_GRAD_SCALE = 21\b", header)
    assert len(L.EXPORTS) == 179
    assert not any(n.startswith(("scn_clip", "scn_grad")) for n in L.EXPORTS)
    assert not re.search(r"\bscn_(clip|grad)\w*\s*\(", header)
    assert re.findall(r"\((\d+) entry\s+(?:\*\s+)?points\)", header)[-1] == "179"
    assert callable(EX.clip_segments)
    lib = L.load()                                              # (no GPU needed: nothing is launched)
    assert lib.scn_exec_struct_bytes(0) == 64 == C.sizeof(EX.ExecOp)
    assert lib.scn_exec_struct_bytes(1) == 136 == C.sizeof(EX.ExecLevel)


def _requirements(counts):
    from sparse_rcnn_amd import _lib as L, executor as EX
    ops, levels, prefix = EX.clip_plan(counts, 1.0, 1.0)
    scratch, arrival = C.c_int64(-1), C.c_int64(-1)
    rc = L.load().scn_exec_requirements(ops, 2, levels, 1, C.byref(scratch), C.byref(arrival))
    return rc, scratch.value, arrival.value


def test_requirements_count_the_partial_sums():
    from sparse_rcnn_amd import executor as EX
    counts = (1, 4097, 0, 12345)
    rc, scratch, arrival = _requirements(counts)
    # documented: 8 bytes per workgroup of the partial-sum launches, one workgroup per 4096-element chunk of a segment
    documented = 8 * sum(-(-n // 4096) for n in counts)
    assert documented == 8 * (1 + 2 + 0 + 4)
    assert rc == 0 and scratch >= documented and arrival == 0
    assert EX.clip_scratch_bytes(counts) >= documented
    big = (5_000_000,)                                          # beyond the executor's 256-byte floor
    rc, scratch, _ = _requirements(big)
    assert rc == 0 and scratch >= 8 * -(-big[0] // 4096) and EX.clip_scratch_bytes(big) >= 8 * -(-big[0] // 4096)
    # the Python side asks the library: one answer, over a sweep of tables around the chunk and the launch split
    rng = np.random.default_rng(0)
    for t in (0, 1, 2, 79, 80, 81, 200):
        counts = [int(n) for n in rng.choice([0, 1, 4095, 4096, 4097, 100_000, 3_000_001], size=t)]
        rc, scratch, _ = _requirements(counts)
        assert rc == 0 and EX.clip_scratch_bytes(counts) == scratch >= max(256, 8 * sum(-(-n // 4096) for n in counts))
        assert EX.clip_launches(counts) == 2 * -(-sum(1 for n in counts if n) // 80) + 1


def test_requirements_refuse_a_negative_count():
    from sparse_rcnn_amd import _lib as L
    rc, _, _ = _requirements((16, -1, 4))
    assert rc == L.EINVAL == 1 and L.load().scn_last_error_string()


def _case(seed, nan=False):
    g = torch.Generator().manual_seed(seed)
    grads = [torch.randn(shape, generator=g, dtype=torch.float64) for shape in ((3, 5), (7,), (1,), (4, 2, 3), (129,))]
    if nan:
        grads[2][0] = float("nan")
    return grads


@pytest.mark.parametrize("which", ["above", "below", "nan"])
def test_the_restatement_agrees_with_torch_in_float64(which):
    grads = _case(5, nan=which == "nan")
    norm = R.total_norm([g.numpy() for g in grads])
    bound = {"above": 2.0 * norm, "below": 0.5 * norm, "nan": 1.0}[which]
    params = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    ref_total = float(torch.nn.utils.clip_grad_norm_(params, bound))
    total, scaled = R.clip_f64([g.numpy() for g in grads], bound)
    if which == "nan":
        assert np.isnan(total) and np.isnan(ref_total)
        assert R.record([g.numpy() for g in grads], bound)[2] == 1.0 and np.isnan(R.record([g.numpy() for g in grads], bound)[1])
        for p, s in zip(params, scaled):
            assert np.isnan(p.grad.numpy()).all() and np.isnan(s).all()
        return
    assert abs(total - ref_total) <= 1e-12 * ref_total
    for p, s, g in zip(params, scaled, grads):
        ref = p.grad.numpy()
        assert np.abs(s - ref).max() <= 1e-12 * np.abs(ref).max()
        if which == "above":
            assert np.array_equal(ref, g.numpy())              # not clipped: torch multiplies by 1
    assert R.record([g.numpy() for g in grads], bound)[2] == 0.0


def test_the_fp32_coefficient():
    assert R.coef_f32(np.float32(4.0), 2.0) == np.float32(2.0) / (np.float32(4.0) + np.float32(1e-6))
    assert R.coef_f32(np.float32(1.0), 2.0) == np.float32(1.0)
    assert R.coef_f32(np.float32(3.0), float("inf")) == np.float32(1.0)
    assert R.coef_f32(np.float32("inf"), 2.0) == np.float32(0.0)
    assert np.isnan(R.coef_f32(np.float32("nan"), 2.0))
    # fp32 squares overflow above 1.8e19; the restated norm of such values is finite
    total, coef, bad = R.record([np.full(100, 1e25, dtype=np.float32)], 1.0)
    assert np.isfinite(total) and abs(float(total) - 1e26) <= 1e26 * 2.0 ** -22 and bad == 0.0 and 0 < coef < 1e-25


def test_scene_step_constructs_describes_and_refuses():
    from sparse_rcnn_amd.trainstep import SceneStep
    st = SceneStep("cfg2", optimizer="adam", max_grad_norm=1.0, **SMALL)
    d = st.describe()
    assert st.max_grad_norm == 1.0 and st.flat.max_grad_norm == 1.0 and st.grad_norm is None
    assert "SCN_OP_GRAD_NORM" in d and "SCN_OP_GRAD_SCALE" in d and "L2 norm 1" in d
    launches = 2 * -(-len(st.flat.params) // 80) + 1            # partial-sum and scale launches per <= 80 tensors + the record
    assert f"{launches} launches per step" in d
    plain = SceneStep("cfg2", optimizer="adam", **SMALL)
    dp = plain.describe()
    assert plain.max_grad_norm is None and plain.flat.max_grad_norm is None and plain.grad_norm is None
    assert "GRAD_NORM" not in dp and "clip" not in dp
    assert d.replace(st._describe_clip(), "") == dp             # one clause more, nothing else
    sgd, sgd_clip = SceneStep("cfg2", **SMALL), SceneStep("cfg2", max_grad_norm=0.5, **SMALL)
    assert hashlib.sha256(sgd.describe().encode()).hexdigest() == DEFAULT_DESCRIBE_SHA256
    assert "SCN_OP_GRAD_NORM" in sgd_clip.describe() and sgd_clip.describe().replace(sgd_clip._describe_clip(), "") == sgd.describe()
    assert plain.flat.flat.numel() == st.flat.flat.numel()
    # the description asks FlatParams which path the update takes: a rank weight sends it through the packed buffer
    assert "gradient tensors where autograd left them" in d and not st.flat.single_rank_step_packs()
    st.flat.rank_weight = 0.5
    assert st.flat.single_rank_step_packs() and "3 launches per step over the packed flat gradient" in st.describe()
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            SceneStep("cfg2", optimizer="adam", max_grad_norm=bad, **SMALL)


def test_a_step_that_trains_nothing_with_parameters_is_refused(monkeypatch):
    from sparse_rcnn_amd.trainstep import SceneStep
    # a trained part without parameters: the segmentation head's are taken away before the flat buffer is built
    orig = SceneStep._build_flat

    def strip(self, n_buckets):
        for p in self._part("segmentation").parameters():
            p.requires_grad_(False)
        return orig(self, n_buckets)
    monkeypatch.setattr(SceneStep, "_build_flat", strip)
    with pytest.raises(ValueError, match="max_grad_norm"):
        SceneStep("cfg3", train=("segmentation",), segmentation_loss=True, max_grad_norm=1.0, **SMALL)


def test_clip_grad_norm_refuses_what_it_does_not_do():
    from sparse_rcnn_amd.optim import clip_grad_norm_
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match="norm_type"):
        clip_grad_norm_([p], 1.0, norm_type=1)
    with pytest.raises(ValueError, match="norm_type"):
        clip_grad_norm_([p], 1.0, norm_type=float("inf"))
    with pytest.raises(ValueError, match="no CPU"):
        clip_grad_norm_([p], 1.0)
    q = torch.nn.Parameter(torch.zeros(4))
    assert float(clip_grad_norm_([q], 1.0)) == 0.0              # no gradient anywhere: torch's zero
