"""CPU: the fixtures of the reference's own loss container (tests/golden/loss_container_*.npz, made by
tests/golden/make_loss_container_golden.py) meet the float64 restatement (tests/loss_container_restate.py) within the derived
bounds; sparse_rcnn_amd.loss.Loss has the reference's parameters and refuses what it does not compute; SceneStep checks its new
arguments before it touches a GPU."""
import glob
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_container_restate as RS                            # noqa: E402

CASES = sorted(glob.glob(os.path.join(HERE, "golden", "loss_container_*.npz")))
KEYS = json.load(open(os.path.join(HERE, "golden", "loss_container_keys.json")))
ID = lambda p: os.path.basename(p)[len("loss_container_"):-4]     # noqa: E731
NEEDED = dict(mask_positive_threshold=0.2, class_positive_threshold=0.1, class_negative_threshold=0, class_negative_label=-100)
ON = dict(calc_bbox=True, calc_class=True, calc_mask=True, calc_segmentation=True)


def test_fixtures_present():
    names = {ID(p) for p in CASES}
    assert {"all_multitask", "all_fixed", "rpn_only", "no_class_mask", "unit_fixed", "unit_multitask", "learned", "no_rpn"} <= names
    z = {ID(p): np.load(p) for p in CASES}
    assert np.allclose(z["all_multitask"]["ctor_weights"], (2, 0.5, 0.25, 4, 0.125))
    assert not z["rpn_only"]["present"][2:].any() and z["rpn_only"]["present"][:2].all()
    assert list(z["no_class_mask"]["present"]) == [True, True, False, False, True]
    assert bool(z["all_multitask"]["multitask"]) and not bool(z["all_fixed"]["multitask"])
    allt = np.concatenate([v["terms"] for v in z.values()])
    assert allt.min() >= 1e-3 and allt.max() <= 10 and allt.min() < 1e-2 and allt.max() > 5       # terms span 1e-3 .. 10
    for p in CASES:
        assert os.path.getsize(p) <= 16 * 1024


@pytest.mark.parametrize("path", CASES, ids=ID)
def test_fixture_meets_the_restatement(path):
    z = np.load(path)
    r = RS.combine(z["terms"], z["present"], z["params"])
    for name, got, ref, s in (("total", z["total"], r["total"], r["S_total"]),
                              ("total_multitask", z["total_multitask"], r["total_multitask"], r["S_multitask"])):
        err = abs(float(got) - ref)
        print(f"{ID(path)} {name}: |err| {err:.3e} bound {RS.bound(s):.3e}")
        assert err <= RS.bound(s), name
    # the parameters are -log(constructor weight), unless the case wrote trained values over them
    if ID(path) != "learned":
        assert np.array_equal(z["params"], (-torch.log(torch.tensor(z["ctor_weights"], dtype=torch.float32))).numpy())
    assert list(z["term_has_grad"]) == list(z["present"])
    for i in range(5):
        if z["present"][i]:
            err = abs(float(z["term_grad"][i]) - r["term_grad"][i])
            assert err <= RS.bound(r["S_term_grad"][i]), (i, err)
    want = r["weight_used"] & bool(z["multitask"])
    assert list(z["weight_has_grad"]) == list(want)
    for j in range(5):
        if want[j]:
            err = abs(float(z["weight_grad"][j]) - r["weight_grad"][j])
            assert err <= RS.bound(r["S_weight_grad"][j]), (j, err)
    keys = ["_total_", "_total_multitask_"] + [n for n, p in zip(RS.TERM_NAMES, z["present"]) if p]
    assert list(z["subloss_keys"]) == keys
    assert np.array_equal(z["subloss_values"][2:], z["terms"][z["present"]])


@pytest.mark.parametrize("path", [p for p in CASES if ID(p).startswith("unit")], ids=ID)
def test_unit_weights_are_the_plain_sum(path):
    z = np.load(path)
    want = RS.plain_sum_f32(z["terms"], z["present"])
    assert z["total"].view(np.int32) == want.view(np.int32)
    assert z["total_multitask"].view(np.int32) == z["total"].view(np.int32)


@pytest.mark.parametrize("name", sorted(KEYS))
def test_parameters_match_the_reference(name):
    from sparse_rcnn_amd.loss import Loss
    k = KEYS[name]
    loss = Loss(batchwise_subsample=True, sparse=True, multitask_loss=k["multitask"], loss_rpn_class_weight=2,
                loss_rpn_bbox_weight=0.5, loss_class_weight=0.25, loss_mask_weight=4, loss_segmentation_weight=0.125,
                **k["calc"], **NEEDED)
    own = {n: p for n, p in loss.named_parameters() if "." not in n}
    assert sorted(own) == sorted(k["parameters"])
    for n, ref in k["parameters"].items():
        p = own[n]
        assert list(p.shape) == ref["shape"] and p.dtype == torch.float32
        assert p.requires_grad == ref["requires_grad"], n
        assert int(p.detach().view(torch.int32)) == ref["bits"], n                    # bit-equal initial values
    assert (loss.rpn_loss is not None) == k["calc"]["calc_bbox"]
    assert (loss.class_loss is not None) == k["calc"]["calc_class"] == (loss.class_loss_selector is not None)
    assert (loss.mask_loss is not None) == k["calc"]["calc_mask"]
    assert (loss.segmentation_loss is not None) == k["calc"]["calc_segmentation"]
    # a reference state_dict (its keys and shapes) maps onto the container completely
    sd = {key: torch.full(shape, 0.25) for key, shape in k["state_dict"].items()}
    assert loss.load_reference_state_dict(sd) == ([], [])
    assert loss.loss_mask_weight.detach().item() == 0.25
    sd2 = {"loss." + key: v for key, v in sd.items()}
    sd2["other.weight"] = torch.zeros(3)
    assert loss.load_reference_state_dict(sd2, prefix="loss.") == ([], [])
    del sd["loss_class_weight"]
    sd["stray"] = torch.zeros(())
    with pytest.raises(KeyError):
        loss.load_reference_state_dict(sd)
    assert loss.load_reference_state_dict(sd, strict=False) == (["loss_class_weight"], ["stray"])


def test_get_weights_has_the_reference_naming():
    from sparse_rcnn_amd.loss import Loss
    z = np.load(os.path.join(HERE, "golden", "loss_container_all_multitask.npz"))
    loss = Loss(batchwise_subsample=True, sparse=True, multitask_loss=True, loss_rpn_class_weight=2, loss_rpn_bbox_weight=0.5,
                loss_class_weight=0.25, loss_mask_weight=4, loss_segmentation_weight=0.125, **ON, **NEEDED)
    gw = loss.get_weights()
    assert list(gw) == list(z["get_weights_keys"]) == ["rpn_score", "rpn_bbox", "class", "mask", "segment"]
    assert np.array_equal(np.array(list(gw.values()), np.float32), z["get_weights_values"])
    assert gw["rpn_score"] == 2.0 and gw["rpn_bbox"] == 0.5                 # exp(-loss_rpn_class_weight), its crossed naming
    rpn = Loss(batchwise_subsample=True, calc_bbox=True, calc_class=False, calc_mask=False, calc_segmentation=False, **NEEDED)
    assert list(rpn.get_weights()) == ["rpn_score", "rpn_bbox"]
    assert rpn.running_means() == {}


def test_refusals():
    from sparse_rcnn_amd.loss import Loss
    with pytest.raises(ValueError, match=r"batchwise_subsample=False \(the reference's default\).*batchwise_subsample=True"):
        Loss(sparse=True, **ON, **NEEDED)
    with pytest.raises(ValueError, match="sparse=False"):
        Loss(batchwise_subsample=True, **ON, **NEEDED)
    for dt in (torch.float64, torch.bfloat16, torch.float16):
        with pytest.raises(ValueError, match="dtype"):
            Loss(batchwise_subsample=True, sparse=True, dtype=dt, **ON, **NEEDED)
    with pytest.raises(ValueError, match="loss_mask_weight"):
        Loss(batchwise_subsample=True, sparse=True, loss_mask_weight=0, **ON, **NEEDED)
    # without the RPN criterion the selector is never built: the reference's default passes
    Loss(sparse=True, calc_bbox=False, calc_class=True, calc_mask=True, calc_segmentation=True, **NEEDED)
    # the selector's keywords reach it, the seed too
    l = Loss(batchwise_subsample=True, sparse=True, seed=9, positive_overlap=0.4, negative_overlap=0.1, max_weight=1 / 4,
             **ON, **NEEDED)
    s = l.rpn_loss.bbox_target_selector
    assert (s.seed, s.positive_overlap, s.negative_overlap, s.min_inverse_weight) == (9, 0.4, 0.1, 4.0)
    # CPU terms: there is no CPU path
    from sparse_rcnn_amd._lib import ScnError
    with pytest.raises(ScnError):
        l.combine([torch.zeros(())] * 5)


def test_scenestep_checks_its_arguments_before_any_gpu_use():
    from sparse_rcnn_amd.trainstep import SceneStep
    cpu = torch.device("cpu")
    four = dict(rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True)
    with pytest.raises(ValueError, match="unknown"):
        SceneStep("cfg3-rpn", device=cpu, loss_weights=dict(rpn=2.0), **four)
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="positive"):
            SceneStep("cfg3-rpn", device=cpu, loss_weights=dict(mask=bad), **four)
    with pytest.raises(ValueError, match="is off"):
        SceneStep("cfg3-rpn", device=cpu, rpn_loss=True, loss_weights=dict(segmentation=0.125))
    with pytest.raises(ValueError, match="is off"):
        SceneStep("cfg3-rpn", device=cpu, segmentation_loss=True, loss_weights=dict(rpn_bbox=0.5))
    with pytest.raises(ValueError, match="loss_weights"):
        SceneStep("cfg3-rpn", device=cpu, loss_weights=[1, 1, 1, 1, 1], **four)
    # like the other loss flags: it needs the losses it weighs, and they need an RPN in the step
    with pytest.raises(ValueError, match="multitask_loss=True needs"):
        SceneStep("cfg3-rpn", device=cpu, multitask_loss=True)
    with pytest.raises(ValueError, match="multitask_loss=True needs"):
        SceneStep("cfg2", device=cpu, multitask_loss=True)
    with pytest.raises(ValueError, match="rpn_loss=True needs an RPN"):
        SceneStep("cfg3", device=cpu, multitask_loss=True, rpn_loss=True)


def test_header_declares_the_new_exports():
    from sparse_rcnn_amd import _lib as L
    header = open(os.path.join(HERE, "..", "include", "scn_mi355x.h")).read()
    for name in ("scn_loss_combine", "scn_loss_combine_bwd"):
        assert name in L.EXPORTS
        assert re.search(r"\bint " + name + r"\(", header), name
    assert len(L.EXPORTS) == 179 and "(177 entry points)" in header and "(178 entry points)" in header
    assert "(179 entry points)" in header                            # (+ scn_conv_tiles_bf16_plan_describe: the count only grows)
    assert re.search(r"#define SCN_LOSS_TERMS " + str(L.LOSS_TERMS) + r"\b", header)
    assert re.search(r"#define SCN_LOSS_RECORD " + str(L.LOSS_RECORD) + r"\b", header)


def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


_PACK_CODE = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
BUCKETS = %d
if BUCKETS:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=%r, RANK="0", WORLD_SIZE="1", SCN_DP_FORCE_BUCKETS="1")
    dist.init_process_group("gloo")
from sparse_rcnn_amd.dp import FlatParams
from sparse_rcnn_amd.loss import LossCombiner
torch.manual_seed(0)
net = torch.nn.Module()
net.a, net.unused, net.b = torch.nn.Linear(3, 4), torch.nn.Linear(5, 5), torch.nn.Linear(4, 2)
net.loss_combiner = LossCombiner((2, 0.5, 1, 1, 0.125), multitask_loss=True)
fp = FlatParams(net, n_buckets=BUCKETS)
assert bool(fp.buckets) == bool(BUCKETS) and len(fp.params) == 11
ws = net.loss_combiner.log_weights()
on = ws[:2] + ws[4:]                                   # the class and mask losses are off: their weights get no gradient
index = {id(p): i for i, p in enumerate(fp.params)}
first = fp.grad_views[index[id(ws[0])]].storage_offset()
x = torch.ones(1, 3)

def micro_batch(k, zero, last):
    """What SceneStep does: views adopted, the kernel's `+=` into them, then autograd's backward."""
    if zero:
        fp.zero_grad()
        fp.flat_grad[first:first + 5].zero_()
    views = fp.adopt_views(on)
    for j, v in enumerate(views):
        v += (j + 1.0) * (k + 1)
    if last:
        fp.mark_ready(on)
    net.b(net.a(x * (k + 1))).sum().backward()

fp.flat_grad.fill_(99.0)                                # stale values everywhere: packing must clear what has no gradient
with fp.accumulate():
    micro_batch(0, True, False)
micro_batch(1, False, True)
assert all(p.grad is None for p in ws[2:4]) and net.unused.weight.grad is None
fp.all_reduce_mean()
g = fp.mean_grad()
got = g[first:first + 5].tolist()
assert got == [3.0, 6.0, 0.0, 0.0, 9.0], got           # both micro-batches, not zeroed with the parameters without a gradient
views = fp.mean_grad_views()
assert views[index[id(net.unused.weight)]].abs().sum() == 0 and views[index[id(net.unused.bias)]].abs().sum() == 0
assert torch.equal(views[index[id(net.a.weight)]], net.a.weight.grad) and net.a.weight.grad.abs().sum() > 0
fp.zero_grad()
assert not fp._in_place and all(p.grad is None for p in ws)
# a step without kernel-filled views packs as before
net.b(net.a(x)).sum().backward()
fp.all_reduce_mean()
assert fp.mean_grad()[first:first + 5].abs().sum() == 0
print("DONE")
'''


@pytest.mark.parametrize("buckets", [0, 2], ids=["plain", "bucketed"])
def test_kernel_filled_gradients_survive_packing_next_to_a_parameter_without_gradient(buckets):
    """The log-weights' `.grad` are views of the flat gradient buffer that a kernel accumulates into.  Packing zeroes for the
    parameters that received no gradient (here: an unused layer and the weights of two losses that are off) and must neither
    zero the kernel-filled views with them nor lose what earlier micro-batches accumulated."""
    code = _PACK_CODE % (os.path.join(HERE, ".."), buckets, str(_free_port()))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DONE" in r.stdout, (r.stdout, r.stderr[-2000:])


def test_flatparams_mark_ready_counts_kernel_filled_gradients_on_the_bucketed_path():
    """The log-weights' gradients are written by a kernel, not by autograd: on the bucketed all-reduce path their post-accumulate
    hooks never fire, so SceneStep counts them through FlatParams.mark_ready.  One gloo rank with forced buckets."""
    code = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=%r, RANK="0", WORLD_SIZE="1", SCN_DP_FORCE_BUCKETS="1")
dist.init_process_group("gloo")
from sparse_rcnn_amd.dp import FlatParams
from sparse_rcnn_amd.loss import LossCombiner
torch.manual_seed(0)
net = torch.nn.Module()
net.a, net.b = torch.nn.Linear(3, 4), torch.nn.Linear(4, 2)
net.loss_combiner = LossCombiner((2, 0.5, 1, 1, 0.125), multitask_loss=True)
fp = FlatParams(net, n_buckets=2)
assert fp.buckets and len(fp.params) == 9
ws = net.loss_combiner.log_weights()
index = {id(p): i for i, p in enumerate(fp.params)}
views = [fp.grad_views[index[id(p)]] for p in ws]
first = views[0].storage_offset()
assert [v.storage_offset() for v in views] == list(range(first, first + 5))      # adjacent, as SceneStep requires
x = torch.ones(1, 3)

def step(mark):
    fp.zero_grad()
    for k, (p, v) in enumerate(zip(ws, views)):
        v.fill_(k + 1.0)
        p.grad = v
    if mark:
        fp.mark_ready(ws)
    net.b(net.a(x)).sum().backward()
    fp.all_reduce_mean()
    return fp.mean_grad().clone()

marked, forced = step(True), step(False)
assert torch.equal(marked, forced)                      # the forced drain at the end gives the same buffer, later
assert marked[first:first + 5].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
assert marked[:first].abs().sum() > 0
fp.zero_grad()
fp.mark_ready(ws)
try:
    fp.mark_ready(ws)
    print("NOT RAISED")
except RuntimeError:
    print("RAISED")
fp.all_reduce_mean()
plain = FlatParams(torch.nn.Linear(2, 2), n_buckets=0)
plain.mark_ready(plain.params)                          # no buckets: nothing to count
print("DONE")
''' % (os.path.join(HERE, ".."), str(_free_port()))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RAISED" in r.stdout and "NOT RAISED" not in r.stdout and "DONE" in r.stdout, \
        (r.stdout, r.stderr[-2000:])
