"""Generates the class / segmentation fixtures by RUNNING the reference's own code (build container only, needs
/root/reference; `import sparseconvnet` is satisfied by this repository's package):

    python tests/golden/make_class_golden.py

  class_loss_*.npz   ndsis/modules/model.py OverlapCalculator -> TrainSelector(0.1, 0, (32, 0, True)) (numpy's generator
                     seeded right before it) -> ClassLossSelector -> ndsis/modules/loss.py ClassLoss, back-propagated to
                     seeded class scores [BB, 18]; case `nodesc` is the branch without selection descriptions
                     (ClassLossSelector(0.1, 0.05, negative_label=17) over all proposals).
  xent_*.npz         nn.CrossEntropyLoss(weight, ignore_index=-100, reduction='mean') forward / backward, and the outputs of
                     the reference's SegmentationPredictor(sparse=True) and ClassPredictor on the same logits.  The logits
                     are `rng.standard_normal((n, c)) * scale` of numpy's default_rng(seed) cast to fp32 (with a checksum);
                     the (4000, 20) cases store every 10th row of gradient and probabilities plus the gradient's norm, to
                     stay under 100 KB.
  dropin_class_network.json   state-dict keys and shapes, census and repr of the reference's ClassNetwork and
                     SegmentationNetwork built on this package.
  stepmodel_params.json (--stepmodel; written at the commit BEFORE the class branch existed and kept): parameter names and
                     shapes of trainstep.SparseStepModel built without the class / segmentation arguments.
Only inputs and outputs are stored.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

K = 18
BIG_ROW_STEP = 10


def xent_logits(seed, n, c, scale):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, c)) * scale).astype(np.float32)
    t = rng.integers(0, c, size=n).astype(np.int64)
    t[rng.uniform(size=n) < 0.2] = -100
    w = rng.uniform(0.2, 3.0, c).astype(np.float32)
    return x, t, w


def stepmodel():
    import sparse_rcnn_amd                                     # noqa: F401
    from sparse_rcnn_amd.trainstep import SparseStepModel, REF_PLAN
    out = {}
    for kind, ch in (("stand-in", (32, 64, 128, 256)), ("reference", REF_PLAN)):
        torch.manual_seed(0)
        m = SparseStepModel(tuple(ch), True, False, kind, 64)
        params = [(n, list(p.shape)) for n, p in m.named_parameters()]
        out[kind] = dict(channels=list(ch), params=params, n_tensors=len(params),
                         n_params=int(sum(p.numel() for p in m.parameters())))
        print(kind, out[kind]["n_tensors"], out[kind]["n_params"])
    with open(os.path.join(HERE, "stepmodel_params.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)


def main():
    sys.path.insert(0, "/root/reference")
    import sparse_rcnn_amd
    sys.modules["sparseconvnet"] = sparse_rcnn_amd
    from ndsis.modules.model import (OverlapCalculator, TrainSelector, ClassLossSelector, ClassPredictor, SegmentationPredictor,
                                     ClassNetwork, SegmentationNetwork, FeatureLevelDescriptor as FLD)
    from ndsis.modules.loss import ClassLoss
    from make_mask_loss_golden import boxes_near, random_boxes

    def class_case(name, seed, grid, n_gt, n_near, n_far, class_weights=False, nodesc=False):
        rng = np.random.default_rng(seed)
        gts, preds, labels = [], [], []
        for b in range(len(n_gt)):
            g = random_boxes(rng, n_gt[b], grid, 3.0, 0.7 * min(grid))
            gts.append(g)
            far = random_boxes(rng, n_far[b], grid, 2.0, 10.0)
            preds.append(np.concatenate([boxes_near(rng, g, n_near[b], 0.45 if nodesc else 0.15), far]))
            labels.append(rng.integers(0, K - 1 if nodesc else K, size=n_gt[b]).astype(np.int64))
        ov = OverlapCalculator()([torch.from_numpy(p) for p in preds], [torch.from_numpy(g) for g in gts])
        cw = torch.from_numpy(rng.uniform(0.2, 3.0, K).astype(np.float32)) if class_weights else None
        out = dict(k=np.array(K), np_seed=np.array(seed), pred_boxes=np.concatenate(preds).reshape(-1, 2, 3),
                   pred_counts=np.array([len(p) for p in preds], np.int64),
                   gt_boxes=np.concatenate(gts).reshape(-1, 2, 3), gt_counts=np.array(n_gt, np.int64),
                   gt_labels=np.concatenate(labels), max_overlap=np.concatenate([t[2].numpy() for t in ov]),
                   argmax=np.concatenate([t[3].numpy() for t in ov]),
                   class_weights=cw.numpy() if cw is not None else np.zeros(0, np.float32), nodesc=np.array(int(nodesc)))
        lt = [torch.from_numpy(l) for l in labels]
        if nodesc:
            counts = [len(p) for p in preds]
            scores = torch.from_numpy((rng.normal(size=(sum(counts), K)) * 2).astype(np.float32)).requires_grad_()
            selector = ClassLossSelector(0.1, 0.05, negative_label=K - 1)
            sel_scores, sel_labels = selector(scores, (None, counts), None, ov, lt)
            keep = torch.cat([selector.loss_filter(t[2], t[3])[0] for t in ov]).numpy()
            full = np.full(sum(counts), -100, np.int64)          # the reference's compacted labels back at their rows
            full[keep] = torch.cat(sel_labels).numpy()
            out.update(keep=keep, labels_full=full, positive_threshold=np.array(0.1), negative_threshold=np.array(0.05),
                       negative_label=np.array(K - 1))
        else:
            np.random.seed(seed)
            fwd, descs = TrainSelector(0.1, 0, (32, 0, True))(ov)
            counts = [len(f) for f in fwd]
            scores = torch.from_numpy((rng.normal(size=(sum(counts), K)) * 2).astype(np.float32)).requires_grad_()
            selector = ClassLossSelector(0.1)
            sel_scores, sel_labels = selector(scores, (None, counts), descs, ov, lt)
            full = torch.cat(sel_labels).numpy()
            out.update(drawn=np.concatenate([np.asarray(d.pred_selection, np.int64).reshape(-1) for d in descs]),
                       drawn_counts=np.array([len(d.pred_selection) for d in descs], np.int64),
                       fwd_boxes=torch.cat(list(fwd)).numpy().reshape(-1, 2, 3),
                       gt_association=torch.cat([d.gt_association for d in descs]).numpy(), labels_full=full,
                       positive_threshold=np.array(0.1), negative_threshold=np.array(0.0), negative_label=np.array(-100))
        loss = ClassLoss(class_weights=cw)(sel_scores, sel_labels)
        loss.backward()
        valid, o = [], 0
        for c in counts:
            valid.append(int((full[o:o + c] >= 0).sum()))
            o += c
        out.update(box_counts=np.array(counts, np.int64), labels=torch.cat(sel_labels).numpy(),
                   label_counts=np.array([len(l) for l in sel_labels], np.int64), scores=scores.detach().numpy(),
                   loss=loss.detach().numpy(), grad=scores.grad.numpy(), valid_counts=np.array(valid, np.int64))
        path = os.path.join(HERE, f"class_loss_{name}.npz")
        np.savez_compressed(path, **out)
        npos = [int((t[2] >= 0.1).sum()) for t in ov]
        print(f"{name}: positives {npos}, rows {counts}, valid rows per sample {valid}, loss {float(loss.detach()):.6g}, "
              f"{os.path.getsize(path)} bytes")

    # (a) more positives than 32 in sample 0, fewer in sample 1
    class_case("basic", 0, (40, 32, 24), [6, 3], [60, 8], [10, 12])
    # (b) class weights, three samples
    class_case("weights", 1, (32, 32, 16), [4, 5, 2], [30, 6, 3], [4, 8, 2], class_weights=True)
    # (c) a sample without ground truth
    class_case("empty", 2, (32, 24, 16), [4, 0, 3], [12, 0, 5], [3, 6, 2])
    # (d) no selection descriptions: negatives are class 17, rows between the thresholds are dropped
    class_case("nodesc", 3, (40, 32, 24), [5, 4], [40, 30], [30, 20], nodesc=True)

    def xent_case(name, seed, n, c, scale, weights, tie=False):
        x, t, w = xent_logits(seed, n, c, scale)
        if tie:
            x[5, 7] = x[5, 3] = x[5].max() + 1.0                 # an exact tie: the first index wins
            x[9, :] = 0.25                                       # a constant row
        xt = torch.from_numpy(x).requires_grad_()
        wt = torch.from_numpy(w) if weights else None
        loss = torch.nn.CrossEntropyLoss(weight=wt, ignore_index=-100, reduction='mean')(xt, torch.from_numpy(t))
        loss.backward()
        seg_class, seg_prob = SegmentationPredictor(True)(xt.detach())
        cls_idx, cls_prob, cls_raw = ClassPredictor()(xt.detach(), (None, [n - n // 2, n // 2]))
        assert torch.equal(torch.cat(cls_idx), cls_raw) and torch.equal(torch.cat(cls_prob), seg_prob)
        grad = xt.grad.numpy()
        step = BIG_ROW_STEP if n > 1000 else 1
        out = dict(seed=np.array(seed), n=np.array(n), c=np.array(c), scale=np.array(float(scale)), row_step=np.array(step),
                   checksum=np.array(x.astype(np.float64).sum()), targets=t,
                   weights=w if weights else np.zeros(0, np.float32), loss=loss.detach().numpy(),
                   grad_rows=grad[::step], grad_norm=np.array(np.sqrt((grad.astype(np.float64) ** 2).sum())),
                   seg_class=seg_class.numpy(), class_indices=cls_raw.numpy(), prob_rows=seg_prob.numpy()[::step],
                   tie=np.array(int(tie)))
        if step == 1:
            out["logits"] = x
        path = os.path.join(HERE, f"xent_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"xent_{name}: n {n} c {c} scale {scale} weights {weights} valid {int((t >= 0).sum())} "
              f"loss {float(loss.detach()):.6g} {os.path.getsize(path)} bytes")

    i = 0
    for n, c in ((300, 18), (4000, 20)):
        for weights in (False, True):
            for scale in (1, 8):
                xent_case(f"{n}x{c}_{'w' if weights else 'u'}_s{scale}", 100 + i, n, c, scale, weights)
                i += 1
    xent_case("tie", 200, 300, 18, 1, False, tie=True)

    common = dict(main_path_relu=False, relu_first=True, bottleneck_divisor=0, drop_input_relu=True, make_dense=False,
                  num_units=1)

    def census(net):
        out = {}
        for m in net.modules():
            if type(m).__module__.startswith("sparse_rcnn_amd"):
                out[type(m).__name__] = out.get(type(m).__name__, 0) + 1
        return out

    fixtures = {}
    for fc in (256, 80):
        inp = [FLD(type='B', channels=32, params={**common, 'stride': 1}, anchor_path=None)]
        outd = [FLD(type='B', channels=ch, params={**common, 'stride': 2}, anchor_path=None) for ch in (64, 128)]
        cn = ClassNetwork(3, True, fc, 8, inp, outd, linear_channels=[64], num_classes=18, raw_scene=False, cut_shape=None,
                          pooling_function_or_none=torch.mean, relu_after_pooling=True, selection_tuple=(32, 0, True),
                          positive_threshold=0.1, negative_threshold=0)
        sd = cn.state_dict()
        fixtures[f"class_{fc}"] = dict(feature_channels=fc, n_params=int(sum(v.numel() for v in sd.values())),
                                       keys={k: list(v.shape) for k, v in sd.items()}, census=census(cn), repr=repr(cn))
        print(f"class_{fc}", len(sd), fixtures[f"class_{fc}"]["n_params"])
    for ch in (32,):
        sn = SegmentationNetwork(3, True, [1], [ch], 20)
        sd = sn.state_dict()
        fixtures[f"segmentation_{ch}"] = dict(channels=ch, n_params=int(sum(v.numel() for v in sd.values())),
                                              keys={k: list(v.shape) for k, v in sd.items()}, census=census(sn), repr=repr(sn))
    with open(os.path.join(HERE, "dropin_class_network.json"), "w") as f:
        json.dump(fixtures, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    if "--stepmodel" in sys.argv:
        stepmodel()
    else:
        main()
