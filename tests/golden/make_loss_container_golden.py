"""Generates tests/golden/loss_container_*.npz and loss_container_keys.json by RUNNING the reference's own loss container,
ndsis/modules/loss.py `Loss`: its criteria and selectors are replaced by stub modules that return seeded leaf scalars, so its
combining code (loss.py:101-191) runs on chosen term values; `combined` is back-propagated to the terms and the five
log-weight parameters.  Run in the build container only (needs /root/reference):

    python tests/golden/make_loss_container_golden.py
"""
import json
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, "/root/reference")
import sparse_rcnn_amd                                         # noqa: E402
sys.modules["sparseconvnet"] = sparse_rcnn_amd
from ndsis.modules.loss import Loss                            # noqa: E402

TERMS = ("rpn_score", "rpn_bbox", "class", "mask", "segmentation")
WEIGHTS = ("loss_rpn_class_weight", "loss_rpn_bbox_weight", "loss_class_weight", "loss_mask_weight",
           "loss_segmentation_weight")
CALC = dict(calc_bbox=True, calc_class=True, calc_mask=True, calc_segmentation=True)
FIXED = dict(batchwise_subsample=True, sparse=True, mask_positive_threshold=0.2, class_positive_threshold=0.1,
             class_negative_threshold=0, class_negative_label=-100)


class _Stub(nn.Module):
    """Returns what it was given, whatever it is called with."""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, *a):
        return self.out


def build(ctor_weights, multitask, calc):
    kw = dict(zip(("loss_rpn_class_weight", "loss_rpn_bbox_weight", "loss_class_weight", "loss_mask_weight",
                   "loss_segmentation_weight"), ctor_weights))
    return Loss(multitask_loss=multitask, **kw, **calc, **FIXED)


def case(name, seed, ctor_weights, multitask, present, calc=CALC, params=None, lo=-3.0, hi=1.0):
    """present: which of the five terms the outputs carry.  params: log-weight values written over the constructor's."""
    g = torch.Generator().manual_seed(seed)
    loss = build(ctor_weights, multitask, calc)
    if params is not None:
        with torch.no_grad():
            for n, v in zip(WEIGHTS, params):
                getattr(loss, n).copy_(torch.tensor(v, dtype=torch.float32))
    # terms spanning 1e-3 .. 10, log-uniform
    t = [(10.0 ** (lo + (hi - lo) * torch.rand((), generator=g))).to(torch.float32).requires_grad_() for _ in TERMS]
    outputs, batch = dict(is_training=True), dict(gt_bbox=None, gt_label=None, gt_mask=None, gt_segmentation=None)
    if present[0] or present[1]:
        assert present[0] and present[1]
        outputs.update(rpn_score=None, rpn_bbox=None, rpn_target_calculator=None)
        loss.rpn_loss = _Stub((t[0], t[1]))
    if present[2]:
        outputs.update(mpn_class=None, mpn_class_coord_selection=None, mpn_class_box_selection=None)
        loss.class_loss_selector, loss.class_loss = _Stub(([1], [1])), _Stub(t[2])
    if present[3]:
        outputs.update(mpn_mask=None, mpn_mask_coord_selection=None, mpn_mask_box_selection=None)
        loss.mask_loss_selector, loss.mask_loss = _Stub(([1], [1], [1])), _Stub(t[3])
    if present[4]:
        outputs.update(spn_segmentation=None)
        loss.segmentation_loss = _Stub(t[4])
    combined, sub = loss(batch, outputs)
    if combined.requires_grad:
        combined.backward()
    assert abs(sub["_total_multitask_"] - float(combined)) == 0
    gw = loss.get_weights()
    out = dict(
        terms=np.array([float(x.detach()) for x in t], np.float32), present=np.array(present, bool),
        ctor_weights=np.array(ctor_weights, np.float64), multitask=np.array(bool(multitask)),
        calc=np.array([calc["calc_bbox"], calc["calc_class"], calc["calc_mask"], calc["calc_segmentation"]], bool),
        params=np.array([float(getattr(loss, n).detach()) for n in WEIGHTS], np.float32),
        total=np.array(sub["_total_"], np.float32), total_multitask=np.array(sub["_total_multitask_"], np.float32),
        term_grad=np.array([0.0 if x.grad is None else float(x.grad) for x in t], np.float32),
        term_has_grad=np.array([x.grad is not None for x in t], bool),
        weight_grad=np.array([0.0 if getattr(loss, n).grad is None else float(getattr(loss, n).grad) for n in WEIGHTS],
                             np.float32),
        weight_has_grad=np.array([getattr(loss, n).grad is not None for n in WEIGHTS], bool),
        subloss_keys=np.array(list(sub)), subloss_values=np.array([sub[k] for k in sub], np.float32),
        get_weights_keys=np.array(list(gw)), get_weights_values=np.array([gw[k] for k in gw], np.float32))
    path = os.path.join(HERE, f"loss_container_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: present {present}, multitask {multitask}, total {float(out['total']):.7g} multitask "
          f"{float(out['total_multitask']):.7g}, keys {list(sub)}, {os.path.getsize(path)} bytes")


def keys():
    out = {}
    for name, calc in (("all", CALC),
                       ("rpn_only", dict(calc_bbox=True, calc_class=False, calc_mask=False, calc_segmentation=False)),
                       ("no_class_mask", dict(calc_bbox=True, calc_class=False, calc_mask=False, calc_segmentation=True)),
                       ("mask_segmentation", dict(calc_bbox=False, calc_class=False, calc_mask=True, calc_segmentation=True))):
        for multitask in (False, True):
            loss = build((2, 0.5, 0.25, 4, 0.125), multitask, calc)
            out[f"{name}_{'multitask' if multitask else 'fixed'}"] = dict(
                calc=calc, multitask=multitask,
                state_dict={k: list(v.shape) for k, v in loss.state_dict().items()},
                parameters={k: dict(shape=list(p.shape), requires_grad=p.requires_grad, value=float(p.detach()),
                                    bits=int(p.detach().view(torch.int32)))
                            for k, p in loss.named_parameters() if "." not in k})
    with open(os.path.join(HERE, "loss_container_keys.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("keys:", {k: sorted(v["state_dict"]) for k, v in out.items() if k.endswith("fixed")})


def main():
    w = (2, 0.5, 0.25, 4, 0.125)
    all5 = (True,) * 5
    case("all_multitask", 0, w, True, all5)
    case("all_fixed", 1, w, False, all5)
    case("rpn_only", 2, w, True, (True, True, False, False, False),
         calc=dict(calc_bbox=True, calc_class=False, calc_mask=False, calc_segmentation=False))
    case("no_class_mask", 3, w, True, (True, True, False, False, True))       # criteria built, outputs without mpn_*
    case("unit_fixed", 4, (1, 1, 1, 1, 1), False, all5)
    case("unit_multitask", 5, (1, 1, 1, 1, 1), True, all5)
    case("learned", 6, w, True, all5, params=(0.7, -1.3, 0.05, -0.4, 2.1))     # parameters after some training
    case("no_rpn", 7, w, True, (False, False, True, True, True),
         calc=dict(calc_bbox=False, calc_class=True, calc_mask=True, calc_segmentation=True))
    keys()


if __name__ == "__main__":
    main()
