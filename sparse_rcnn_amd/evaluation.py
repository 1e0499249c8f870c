"""The reference's evaluation (ndsis/training/evaluation.py) on the device: overlaps, matching, AP / mAP, confusion.

Same class names and call signatures as the reference, device tensors in, so that `training.py`'s AccumulatorCollection runs
on it.  The kernels are csrc/scn_eval.hip (include/scn_mi355x.h: scn_eval_*); there is no CPU path.

What differs from the reference, on purpose:

* Masks never exist as fp32 or bool matrices on the hot path.  A prediction may be given as the reference's dense fp32
  [P, N] tensor (packed by scn_eval_pack_threshold) or already packed (`mask_bits`, `PackedSample`); ground truth as a bool
  [G, N] tensor or packed (`loss.PackedMasks` / `split_packed`).  The IoU is a popcount contraction of 32-bit words; every
  value is one correctly rounded fp32 division of two exact integers and equals the reference's bit for bit, NaN for 0 / 0
  included.
* A calculator called directly returns the reference's compacted tensors, whose shapes depend on the scores: that call waits
  for the host.  The accumulators do not go through it: they keep the unfiltered matrices and a keep-flag per prediction on
  the device, and wait for the host ONCE, in `get_pr_curve` / `EvaluationHelper.__call__` (one scn_eval_match launch per
  accumulator for all samples x (1 + classes) x thresholds, then one copy of the flags, scores and counts).
* TIE ORDER.  The reference sorts the data set's scores with `score.sort(descending=True)`, whose order of equal scores is
  an accident of the sorting kernel (neither stable nor reversed), and its `gtmask` / `gtlabelmask` curves use a pseudo-score
  of 1 for every prediction.  Here every sort is STABLE: equal scores keep accumulation order (sample-major, prediction order
  inside a sample).
* `EvaluationHelper`'s default class names are the class indices themselves (the reference's `DefaultNames` is not
  subscriptable and raises TypeError).  `raw_pr_curves` is not produced (an empty dict is returned in its place).
"""
from __future__ import annotations

from itertools import chain
import numpy as np
import torch

from . import _lib as L
from .loss import PackedMasks, pack_gt_masks

__all__ = ["PackedSample", "split_packed", "mask_bits", "pack_threshold", "mask_iou", "bbox_iou", "match",
           "OverlapCalculator", "MaskOverlapCalculator", "BboxOverlapCalculator", "OverlapAccumulator",
           "ClasswiseOverlapAccumulator", "PrecisionRecallCurveClassCollection", "PrecisionRecallCurve", "average_precision",
           "metric_key", "EvaluationHelper",
           "BinaryMaskConfusionCalculator", "BinaryConfusionAccumulator", "ConfusionCalculator", "ConfusionAccumulator",
           "ConfusionMatrix", "BinaryConfusionMatrixCollection"]

MATCH_MAX_GT = 4096                        # csrc/scn_eval.hip kMatchMaxGt
CONFUSION_MAX_CLASSES = 64                 # csrc/scn_eval.hip kConfMaxClasses


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _need_cuda(t, name):
    if not torch.is_tensor(t):
        raise ValueError(f"{name}: a tensor is required, got {type(t).__name__}")
    if not t.is_cuda:
        raise L.ScnError(f"{name}: a GPU tensor is required (there is no CPU path)")
    return t


def _host_offsets(counts):
    ho = L.host_i64(len(counts) + 1)
    acc = 0
    for i, c in enumerate(counts):
        acc += int(c)
        ho[i + 1] = acc
    return ho


# ---- packed masks ---------------------------------------------------------------------------------------------------------
class PackedSample:
    """The packed masks of ONE sample: `rows` masks over `n_points` point rows, [rows][ceil(n_points / 32)] words starting at
    word `word_offset` of the int32 device tensor `base` (uint32 bit patterns; bit p % 32 of word p / 32 = point row p; the bits
    beyond n_points are zero).  Samples that share `base` go to the device in one launch without a copy."""

    def __init__(self, base, word_offset, rows, n_points):
        self.base, self.word_offset, self.rows, self.n_points = base, int(word_offset), int(rows), int(n_points)

    @property
    def n_words(self):
        return (self.n_points + 31) // 32

    @property
    def words(self):
        return self.base[self.word_offset:self.word_offset + self.rows * self.n_words].view(self.rows, self.n_words)

    def __len__(self):
        return self.rows

    def unpack(self):
        """bool device [rows, n_points] (for checks)."""
        w = self.words
        bits = (w.unsqueeze(-1) >> torch.arange(32, device=w.device, dtype=torch.int32)) & 1
        return bits.reshape(self.rows, self.n_words * 32)[:, :self.n_points].bool()


def split_packed(packed: PackedMasks):
    """loss.PackedMasks (a batch) -> list of PackedSample views, one per sample."""
    return [PackedSample(packed.words, packed.word_offsets[s], packed.n_gt[s], packed.n_points[s]) for s in range(len(packed))]


def mask_bits(mask_output, sel, box_sample_count, batch_splits, class_indices, num_valid=0, mask_threshold=0.5) -> PackedMasks:
    """`roi.mask_predict(...) > mask_threshold` without the dense masks: mask logits [M, K] over the selection's rows ->
    PackedMasks, sample s's [boxes_s][ceil(N_s / 32)] words (n_gt holds the box counts).  Bit for bit the same decision:
    scn_eval_mask_bits thresholds the sigmoid expression scn_mask_scatter writes.  One memset and one launch; the per-box bit
    offsets (and `class_indices`, if given on the host) go up with small pageable host-to-device copies, as roi.mask_predict's
    row offsets do."""
    from . import roi
    S = _need_cuda(mask_output.detach(), "mask_output")
    if S.dtype != torch.float32:
        S = S.float()
    S = S.contiguous()
    counts, splits, sample, box_start, point_start = roi._box_layout(sel, box_sample_count, batch_splits)
    out = PackedMasks(None, [int(c) for c in counts], [int(n) for n in splits])
    n_words = out.word_offsets[-1]
    out.words = torch.empty(max(n_words, 1), dtype=torch.int32, device=S.device)
    m = int(sel.src_row.shape[0])
    if m and S.shape[0] != m:
        raise L.ScnError(f"mask_output has {S.shape[0]} rows, the selection {m}")
    if S.dim() != 2 or S.shape[1] < 1:
        raise ValueError("mask_output: [M, K] logits required")
    box = np.arange(sel.n_boxes)
    w = (splits + 31) // 32
    bit_base = (np.asarray(out.word_offsets[:-1], np.int64)[sample] + (box - box_start[sample]) * w[sample]) * 32 \
        - point_start[sample]
    cls = torch.as_tensor(class_indices, dtype=torch.int64).to(S.device).contiguous()
    if cls.numel() != sel.n_boxes:
        raise L.ScnError(f"class_indices has {cls.numel()} entries, the selection {sel.n_boxes} boxes")
    bb = torch.from_numpy(np.ascontiguousarray(bit_base, np.int64)).to(S.device)
    L.check(L.lib().scn_eval_mask_bits(L.ptr(S), m, S.shape[1], L.ptr(sel.src_row), L.ptr(sel.box_of), L.ptr(cls),
                                       int(num_valid), float(mask_threshold), L.ptr(bb), sel.n_boxes, n_words,
                                       L.ptr(out.words), L.stream()))
    return out


def pack_threshold(mask_list, mask_threshold=0.5) -> PackedMasks:
    """list of dense fp32 device [P_s, N_s] masks (the reference's outputs['mask']) -> PackedMasks of `mask > mask_threshold`.
    One launch per sample, one buffer."""
    ms = []
    for i, m in enumerate(mask_list):
        _need_cuda(m, f"mask[{i}]")
        if m.dim() != 2:
            raise ValueError(f"mask[{i}]: [P, N] required")
        ms.append(m.detach().float().contiguous())
    dev = ms[0].device if ms else _device()
    out = PackedMasks(None, [int(m.shape[0]) for m in ms], [int(m.shape[1]) for m in ms])
    out.words = torch.empty(max(out.word_offsets[-1], 1), dtype=torch.int32, device=dev)
    for s, m in enumerate(ms):
        L.check(L.lib().scn_eval_pack_threshold(L.ptr(m), m.shape[0], m.shape[1], float(mask_threshold),
                                                out.words.data_ptr() + 4 * out.word_offsets[s], L.stream()))
    return out


def _packed_list(items, name, threshold=None):
    """list whose members are PackedSample / dense tensors (fp32 with `threshold`, else bool / uint8), or a PackedMasks
    -> list of PackedSample."""
    if isinstance(items, PackedMasks):
        return split_packed(items)
    items = list(items)
    dense = [i for i, m in enumerate(items) if not isinstance(m, PackedSample)]
    if dense:
        for i in dense:
            _need_cuda(items[i], f"{name}[{i}]")
        if threshold is not None:
            packed = pack_threshold([items[i] for i in dense], threshold)
        else:
            packed = pack_gt_masks([items[i] if items[i].dtype in (torch.bool, torch.uint8) else items[i] != 0 for i in dense])
        for i, ps in zip(dense, split_packed(packed)):
            items[i] = ps
    return items


def _one_buffer(samples):
    """-> (int32 device tensor, host word offsets) holding every sample; a view when they share their base."""
    if not samples:
        return torch.zeros(1, dtype=torch.int32, device=_device()), L.host_i64(1)
    base = samples[0].base
    offs = L.host_i64(len(samples))
    if all(s.base is base or (s.base.data_ptr() == base.data_ptr()) for s in samples):
        for i, s in enumerate(samples):
            offs[i] = s.word_offset
        return base, offs
    acc = 0
    for i, s in enumerate(samples):
        offs[i] = acc
        acc += s.rows * s.n_words
    return torch.cat([s.words.reshape(-1) for s in samples] + [base.new_zeros(1)]), offs


class MaskIou:
    """Result of `mask_iou`: flat device tensors over the batch; `sample(s)` gives sample s's views."""

    def __init__(self, inter, pred_count, gt_count, iou, confusion, n_pred, n_gt):
        self.inter, self.pred_count, self.gt_count, self.iou, self.confusion = inter, pred_count, gt_count, iou, confusion
        self.n_pred, self.n_gt = list(n_pred), list(n_gt)
        self.pred_off = np.concatenate([[0], np.cumsum(self.n_pred)]).astype(np.int64)
        self.gt_off = np.concatenate([[0], np.cumsum(self.n_gt)]).astype(np.int64)
        self.pair_off = np.concatenate([[0], np.cumsum(np.asarray(self.n_pred, np.int64) * np.asarray(self.n_gt, np.int64))])

    def sample(self, s):
        p, g = self.n_pred[s], self.n_gt[s]
        a, b = int(self.pair_off[s]), int(self.pair_off[s + 1])
        out = dict(inter=self.inter[a:b].view(p, g), iou=self.iou[a:b].view(p, g),
                   pred_count=self.pred_count[int(self.pred_off[s]):int(self.pred_off[s + 1])],
                   gt_count=self.gt_count[int(self.gt_off[s]):int(self.gt_off[s + 1])])
        if self.confusion is not None:
            out["confusion"] = self.confusion[int(self.pred_off[s]):int(self.pred_off[s + 1])]
        return out


def mask_iou(pred, gt, pair_confusion=False) -> MaskIou:
    """Packed predictions x packed ground truth for a batch in one call (scn_eval_mask_iou): `pred`, `gt` lists of
    PackedSample (or PackedMasks).  -> MaskIou: inter int32, |pred|, |gt| int32, iou fp32 = float(inter) / float(union), and
    with `pair_confusion` (needs as many predictions as ground truths per sample) the reference's mask_confusion_pair
    [[tp, fp], [fn, tn]] int64 of prediction i against ground truth i."""
    pred, gt = _packed_list(pred, "pred"), _packed_list(gt, "gt")
    if len(pred) != len(gt):
        raise ValueError(f"{len(pred)} samples of predictions, {len(gt)} of ground truth")
    for s, (a, b) in enumerate(zip(pred, gt)):
        if a.n_points != b.n_points:
            raise L.ScnError(f"sample {s}: predictions over {a.n_points} points, ground truth over {b.n_points}")
        if pair_confusion and a.rows != b.rows:
            raise L.ScnError(f"sample {s}: pair confusion needs as many predictions ({a.rows}) as ground truths ({b.rows})")
    B = len(pred)
    n_pred, n_gt = [a.rows for a in pred], [b.rows for b in gt]
    pw, pwo = _one_buffer(pred)
    gw, gwo = _one_buffer(gt)
    dev = pw.device
    po, go = _host_offsets(n_pred), _host_offsets(n_gt)
    pairs = _host_offsets([p * g for p, g in zip(n_pred, n_gt)])
    inter = torch.empty(pairs[B], dtype=torch.int32, device=dev)
    iou = torch.empty(pairs[B], dtype=torch.float32, device=dev)
    pc = torch.empty(po[B], dtype=torch.int32, device=dev)
    gc = torch.empty(go[B], dtype=torch.int32, device=dev)
    conf = torch.zeros((po[B], 2, 2), dtype=torch.int64, device=dev) if pair_confusion else None
    npt = (L.i64 * max(B, 1))(*[a.n_points for a in pred])
    L.check(L.lib().scn_eval_mask_iou(L.ptr(pw), pwo, L.ptr(gw), gwo, po, go, pairs, npt, B, L.ptr(inter), L.ptr(pc),
                                      L.ptr(gc), L.ptr(iou), L.ptr(conf), L.stream()))
    return MaskIou(inter, pc, gc, iou, conf, n_pred, n_gt)


def _boxes(b, name):
    _need_cuda(b, name)
    if b.dim() != 3 or tuple(b.shape[1:]) != (2, 3):
        raise ValueError(f"{name}: [n, 2, 3] (start, stop) boxes required, got {tuple(b.shape)}")
    return b.detach().float().contiguous()


def bbox_iou(pred_list, gt_list):
    """bbox_overlap_prediction for a batch in one launch: lists of fp32 device [n, 2, 3] boxes -> list of fp32 [P_s, G_s],
    bit-equal to the reference (the device function of the mask loss's overlap kernel)."""
    preds = [_boxes(b, f"pred_bbox[{i}]") for i, b in enumerate(pred_list)]
    gts = [_boxes(b, f"gt_bbox[{i}]") for i, b in enumerate(gt_list)]
    if len(preds) != len(gts):
        raise ValueError(f"{len(preds)} samples of predictions, {len(gts)} of ground truth")
    B = len(preds)
    dev = preds[0].device if preds else _device()
    n_pred, n_gt = [int(b.shape[0]) for b in preds], [int(b.shape[0]) for b in gts]
    po, go = _host_offsets(n_pred), _host_offsets(n_gt)
    pairs = _host_offsets([p * g for p, g in zip(n_pred, n_gt)])
    pf = torch.cat(preds) if B > 1 else (preds[0] if B else torch.empty((0, 2, 3), device=dev))
    gf = torch.cat(gts) if B > 1 else (gts[0] if B else torch.empty((0, 2, 3), device=dev))
    iou = torch.empty(pairs[B], dtype=torch.float32, device=dev)
    L.check(L.lib().scn_eval_bbox_iou(L.ptr(pf), po, L.ptr(gf), go, pairs, B, L.ptr(iou), L.stream()))
    return [iou[pairs[s]:pairs[s + 1]].view(n_pred[s], n_gt[s]) for s in range(B)]


def match(iou_list, thresholds, keep_list=None, pred_class_list=None, gt_class_list=None, classes=None):
    """calc_tp_indicator for every (sample, class or all classes, threshold) in ONE launch (scn_eval_match).  Nothing comes back to the host; the
    problem table (two small arrays) goes up with pageable host-to-device copies, which hold the host until they are issued.
    iou_list: fp32 device [P_s, G_s]; keep_list: None or per sample a bool / uint8 [P_s] flag (None: all kept); classes: the
    class indices of the class-wise problems (needs the class lists), None: classless problems only.
    -> (flags int8 device [n_class_slots, n_thresholds, sum P] with -1 = not part of the problem, 0 = false positive, 1 = true
    positive; num_gt int32 device [n_class_slots, n_thresholds, B]); class slot 0 is "all classes", slot 1 + i is classes[i].
    A problem's predictions are walked in their given order; the first index wins a tie; a NaN among the remaining ground
    truths makes the prediction a false positive (torch's max returns the NaN)."""
    B = len(iou_list)
    dev = iou_list[0].device if B else _device()
    for i, m in enumerate(iou_list):
        _need_cuda(m, f"iou[{i}]")
    n_pred, n_gt = [int(m.shape[0]) for m in iou_list], [int(m.shape[1]) for m in iou_list]
    if n_gt and max(n_gt) > MATCH_MAX_GT:
        raise L.ScnError(f"scn_eval_match serves at most {MATCH_MAX_GT} ground truths per sample, got {max(n_gt)}")
    cls = [-1] + ([int(c) for c in classes] if classes is not None else [])
    thr = [float(t) for t in thresholds]
    sum_p = sum(n_pred)
    po = np.concatenate([[0], np.cumsum(n_pred)]).astype(np.int64)
    go = np.concatenate([[0], np.cumsum(n_gt)]).astype(np.int64)
    pairs = np.concatenate([[0], np.cumsum(np.asarray(n_pred, np.int64) * np.asarray(n_gt, np.int64))]).astype(np.int64)
    nq = len(cls) * len(thr) * B
    n_flags = len(cls) * len(thr) * sum_p
    flags = torch.empty(max(n_flags, 1), dtype=torch.int8, device=dev)[:n_flags].view(len(cls), len(thr), sum_p)
    num_gt = torch.zeros((len(cls), len(thr), B), dtype=torch.int32, device=dev)
    if nq == 0:
        return flags, num_gt
    iou = torch.cat([m.detach().float().reshape(-1) for m in iou_list] + [torch.zeros(1, device=dev)])
    keep = None
    if keep_list is not None and any(k is not None for k in keep_list):
        keep = torch.cat([torch.ones(n_pred[s], dtype=torch.uint8, device=dev) if k is None else k.to(torch.uint8).reshape(-1)
                          for s, k in enumerate(keep_list)] + [torch.zeros(1, dtype=torch.uint8, device=dev)])
    pcl = gcl = None
    if len(cls) > 1:
        if pred_class_list is None or gt_class_list is None or any(c is None for c in chain(pred_class_list, gt_class_list)):
            raise ValueError("class-wise problems need pred_class and gt_class of every sample")
        z = torch.zeros(1, dtype=torch.int64, device=dev)
        pcl = torch.cat([c.to(torch.int64).reshape(-1) for c in pred_class_list] + [z])
        gcl = torch.cat([c.to(torch.int64).reshape(-1) for c in gt_class_list] + [z])
        if pcl.numel() != sum_p + 1 or gcl.numel() != int(go[-1]) + 1:
            raise L.ScnError("pred_class / gt_class do not match the overlap matrices")
    # the problem table: one int64 host array, one copy
    ci, ti, si = np.meshgrid(np.arange(len(cls)), np.arange(len(thr)), np.arange(B), indexing="ij")
    table = np.concatenate([po, go, pairs, np.asarray(cls, np.int64)[ci.reshape(-1)],
                            ((ci * len(thr) + ti) * sum_p + po[si]).reshape(-1).astype(np.int64)])
    t64 = torch.from_numpy(table).to(dev)
    t32 = torch.from_numpy(np.concatenate([si.reshape(-1).astype(np.int32),
                                           np.asarray(thr, np.float32)[ti.reshape(-1)].view(np.int32)])).to(dev)
    b1 = B + 1
    p64, p32 = t64.data_ptr(), t32.data_ptr()
    L.check(L.lib().scn_eval_match(L.ptr(iou), p64, p64 + 8 * b1, p64 + 16 * b1, B, max(n_gt), L.ptr(keep), L.ptr(pcl),
                                   L.ptr(gcl), p32, p64 + 24 * b1, p32 + 4 * nq, p64 + 24 * b1 + 8 * nq, nq,
                                   1 if len(cls) > 1 else 0, flags.untyped_storage().data_ptr() + flags.storage_offset(),
                                   L.ptr(num_gt), L.stream()))
    return flags, num_gt


# ---- overlap calculators ----------------------------------------------------------------------------------------------------
class OverlapCalculator:
    """evaluation.py:12-83.  `iou_batch(pred_list, gt_list)` -> (list of fp32 device [P_s, G_s], list of extra keep flags or
    None).  Called directly it returns the reference's compacted (score, iou, pred_class) and waits for the host; the
    accumulators use `records`, which does not."""

    def __init__(self, score_threshold=None, sort=False):
        self.score_threshold, self.sort = score_threshold, sort

    def iou_batch(self, pred_list, gt_list):
        raise NotImplementedError

    def records(self, score_list, pred_list, gt_list, pred_class_list=None, gt_class_list=None):
        """Per sample a dict(score, iou, keep, pred_class, gt_class) of device tensors, unfiltered: `keep` (uint8 [P] or None)
        is the score / empty-mask filter as a flag; with `sort` the rows are in stable descending score order."""
        score_list = [_need_cuda(s, f"score[{i}]").detach() for i, s in enumerate(score_list)]
        iou_list, extra = self.iou_batch(pred_list, gt_list)
        out = []
        for s, (score, iou) in enumerate(zip(score_list, iou_list)):
            if score.shape[0] != iou.shape[0]:
                raise L.ScnError(f"sample {s}: {score.shape[0]} scores, {iou.shape[0]} predictions")
            pc = pred_class_list[s] if pred_class_list is not None else None
            gc = gt_class_list[s] if gt_class_list is not None else None
            if pc is not None:
                pc = _need_cuda(pc, f"pred_class[{s}]")
            if gc is not None:
                gc = _need_cuda(gc, f"gt_class[{s}]")
            keep = extra[s] if extra is not None else None
            if self.score_threshold is not None:
                k = (score >= self.score_threshold)
                keep = k if keep is None else (keep.bool() & k)
            if self.sort:
                score, order = score.sort(descending=True, stable=True)
                iou = iou[order]
                keep = keep[order] if keep is not None else None
                pc = pc[order] if pc is not None else None
            out.append(dict(score=score, iou=iou, keep=None if keep is None else keep.to(torch.uint8), pred_class=pc,
                            gt_class=gc))
        return out

    def __call__(self, score, pred, gt, pred_class=None):
        r = self.records([score], [pred], [gt], None if pred_class is None else [pred_class])[0]
        score, iou, pc = r["score"], r["iou"], r["pred_class"]
        if r["keep"] is not None:
            k = r["keep"].bool()
            score, iou = score[k], iou[k]
            pc = pc[k] if pc is not None else None
        return score, iou, pc


class MaskOverlapCalculator(OverlapCalculator):
    """evaluation.py:86-148.  pred: dense fp32 [P, N] (thresholded at mask_threshold) or a PackedSample (what `mask_bits`
    made: already thresholded); gt: bool [G, N] or a PackedSample.  filter_masks drops predictions with |pred| = 0."""

    def __init__(self, mask_threshold=0.5, score_threshold=None, sort=False, filter_masks=False):
        super().__init__(score_threshold=score_threshold, sort=sort)
        self.mask_threshold, self.filter_masks = mask_threshold, filter_masks

    def iou_batch(self, pred_list, gt_list):
        r = mask_iou(_packed_list(pred_list, "pred", self.mask_threshold), _packed_list(gt_list, "gt"))
        per = [r.sample(s) for s in range(len(r.n_pred))]
        return [p["iou"] for p in per], ([p["pred_count"] > 0 for p in per] if self.filter_masks else None)


class BboxOverlapCalculator(OverlapCalculator):
    """evaluation.py:151-190: pred / gt fp32 [n, 2, 3] (start, stop) boxes."""

    def iou_batch(self, pred_list, gt_list):
        return bbox_iou(pred_list, gt_list), None


# ---- accumulators and curves ------------------------------------------------------------------------------------------------
class OverlapAccumulator:
    """evaluation.py:193-318.  Keeps the samples' records on the device (`device` is accepted and ignored: nothing moves to
    the host before the curves are asked for)."""

    def __init__(self, overlap_calculator, device=None):
        self.overlap_calculator = overlap_calculator
        self.records = []
        self._cache = {}

    def add_sample(self, score, pred, gt, pred_class=None, gt_class=None):
        self.add_batch([score], [pred], [gt], None if pred_class is None else [pred_class],
                       None if gt_class is None else [gt_class])

    def add_batch(self, score, pred, gt, pred_class=None, gt_class=None):
        """One IoU launch for the batch; no result is read back on the host."""
        if (pred_class is None) != (gt_class is None):
            raise ValueError("pred_class and gt_class are given together or not at all")
        self.records += self.overlap_calculator.records(list(score), pred, gt, pred_class, gt_class)
        self._cache = {}

    # the reference's list attributes, in its compacted form (each waits for the host)
    def _compact(self, key):
        out = []
        for r in self.records:
            t = r[key]
            out.append(t if (t is None or r["keep"] is None) else t[r["keep"].bool()])
        return out

    score_list = property(lambda self: self._compact("score"))
    iou_list = property(lambda self: self._compact("iou"))
    pred_class_list = property(lambda self: self._compact("pred_class"))
    gt_class_list = property(lambda self: [r["gt_class"] for r in self.records])

    def has_classes(self):
        return all(r["pred_class"] is not None for r in self.records)

    def get_counts(self):
        """[(kept predictions, ground truths)] per sample (waits for the host)."""
        return np.array([[int(r["score"].shape[0] if r["keep"] is None else r["keep"].sum().item()), int(r["iou"].shape[1])]
                         for r in self.records]).reshape(-1, 2)

    def matched(self, thresholds, classes=None):
        """All matching problems of this accumulator in one launch and ONE wait for the host.
        -> {(class or None, threshold): (sorted_score fp32 CPU, sorted_tp bool CPU, num_gt)}, sorted by score, descending and
        STABLE (equal scores keep sample-major accumulation order)."""
        key = (tuple(float(t) for t in thresholds), None if classes is None else tuple(int(c) for c in classes))
        if key in self._cache:
            return self._cache[key]
        recs = self.records
        thr, cls = list(key[0]), ([] if key[1] is None else list(key[1]))
        out = {}
        sum_p = sum(int(r["score"].shape[0]) for r in recs)
        B = len(recs)
        if B and thr:
            flags, num_gt = match([r["iou"] for r in recs], thr, [r["keep"] for r in recs],
                                  [r["pred_class"] for r in recs] if cls else None,
                                  [r["gt_class"] for r in recs] if cls else None, cls if cls else None)
            score = torch.cat([r["score"].float().reshape(-1) for r in recs])
            blob = torch.cat([score.view(torch.uint8), num_gt.reshape(-1).view(torch.uint8),
                              flags.reshape(-1).view(torch.uint8)]).cpu().numpy()        # the one wait
            score = blob[:4 * sum_p].view(np.float32)
            n_ng = (1 + len(cls)) * len(thr) * B
            num_gt = blob[4 * sum_p:4 * sum_p + 4 * n_ng].view(np.int32).reshape(1 + len(cls), len(thr), B)
            flags = blob[4 * sum_p + 4 * n_ng:].view(np.int8).reshape(1 + len(cls), len(thr), sum_p)
        for ci, c in enumerate([None] + cls):
            for ti, t in enumerate(thr):
                if B:
                    f = flags[ci, ti]
                    sel = f >= 0
                    sc, tp, ng = score[sel], f[sel] > 0, int(num_gt[ci, ti].sum())
                else:
                    sc, tp, ng = np.zeros(0, np.float32), np.zeros(0, bool), 0
                order = np.argsort(-sc, kind="stable")
                out[(c, t)] = (torch.from_numpy(sc[order].copy()), torch.from_numpy(tp[order].copy()), ng)
        self._cache[key] = out
        return out

    def get_pr_curve(self, overlap_threshold, device=None):
        s, tp, ng = self.matched([overlap_threshold])[(None, float(overlap_threshold))]
        return PrecisionRecallCurve(s.to(device), tp.to(device), ng)

    def get_classwise_accumulator(self, classes, device=None):
        return ClasswiseOverlapAccumulator(self, classes, device)


class ClasswiseOverlapAccumulator:
    """evaluation.py:321-418: the parent's overlaps separated by predicted and ground-truth class.  Nothing is copied: the
    separation is the class argument of the matching problems."""

    def __init__(self, accumulator, classes, device=None, thresholds=None):
        self.accumulator, self.device = accumulator, device
        self.classes = [int(c) for c in (classes.tolist() if torch.is_tensor(classes) else classes)]
        self.thresholds = thresholds

    def get_pr_collection(self, overlap_threshold, device=None):
        thr = self.thresholds if self.thresholds is not None and float(overlap_threshold) in [float(t) for t in self.thresholds] \
            else [overlap_threshold]
        m = self.accumulator.matched(thr, self.classes)
        dev = device if device is not None else self.device
        curves = []
        for c in self.classes:
            s, tp, ng = m[(c, float(overlap_threshold))]
            curves.append(PrecisionRecallCurve(s.to(dev), tp.to(dev), ng))
        return PrecisionRecallCurveClassCollection(curves)

    def get_class_counts(self):
        """[classes][samples] (kept predictions of the class, ground truths of the class) (waits for the host)."""
        out = []
        for c in self.classes:
            row = []
            for r in self.accumulator.records:
                k = r["pred_class"] == c
                if r["keep"] is not None:
                    k = k & r["keep"].bool()
                row.append([int(k.sum().item()), int((r["gt_class"] == c).sum().item())])
            out.append(row)
        return np.array(out)


class PrecisionRecallCurveClassCollection(list):
    """One PrecisionRecallCurve per class (the reference's container of the same name)."""

    def _aps(self, num_samples, no_gt_is_zero):
        return [average_precision(curve, num_samples, no_gt_is_zero) for curve in self]

    def get_ap_list_interpolated_all_points(self, no_gt_is_zero=False):
        return self._aps(None, no_gt_is_zero)

    def get_ap_list_interpolated_sampled(self, num_samples=11, no_gt_is_zero=False):
        return self._aps(num_samples, no_gt_is_zero)

    def get_map_interpolated_all_points(self):
        """Mean over the classes that have ground truth (NaN entries are skipped)."""
        return _nanmean(torch.stack(self._aps(None, False)).cpu().numpy())

    def get_map_interpolated_sampled(self, num_samples=11):
        return _nanmean(torch.stack(self._aps(num_samples, False)).cpu().numpy())


class PrecisionRecallCurve:
    """The precision-recall curve of a score-sorted true-positive indicator.  With h_i = the number of true positives among
    the first i predictions: precision_i = h_i / i, recall_i = h_i / num_gt (one fp32 division of exact integers each), and
    precision_interpolated_i = max over j >= i of precision_j.  A few thousand elements at most: plain torch on the host
    copy."""

    @staticmethod
    def calc_tp_indicator(iou_sorted_by_score, overlap_threshold):
        """One matching problem on the device (scn_eval_match) -> bool [P] on the device; no result is read back."""
        flags, _ = match([iou_sorted_by_score], [overlap_threshold])
        return flags[0, 0] > 0

    def __init__(self, sorted_score, sorted_tp_indicator, num_gt):
        dtype = sorted_score.dtype if sorted_score.is_floating_point() else torch.float32
        hits = torch.cumsum(sorted_tp_indicator.to(dtype), 0)
        rank = torch.arange(1, hits.numel() + 1, dtype=dtype, device=hits.device)
        self.score, self.tp_indicator, self.num_gt = sorted_score, sorted_tp_indicator, num_gt
        self.precision = hits / rank
        self.recall = hits / num_gt                              # (NaN throughout when there is no ground truth)
        self.precision_interpolated = self.precision
        if hits.numel():                                         # running maximum taken from the last rank backwards
            self.precision_interpolated = torch.cummax(self.precision.flip(0), 0).values.flip(0)

    def _scalar(self, value):
        return torch.tensor(value, dtype=self.recall.dtype, device=self.recall.device)

    def get_ap_interpolated_all_points(self, no_gt_is_zero=False):
        """Area under the interpolated curve: sum_i (recall_i - recall_{i-1}) * precision_interpolated_i, recall_0 = 0.  No
        prediction: 0 if there is ground truth (or no_gt_is_zero), else NaN."""
        if self.recall.numel() == 0:
            return self._scalar(0.0 if (self.num_gt or no_gt_is_zero) else float("nan"))
        step = torch.diff(self.recall, prepend=self.recall.new_zeros(1))
        return torch.sum(step * self.precision_interpolated)

    def get_ap_interpolated_sampled(self, num_samples=11, no_gt_is_zero=False):
        """Mean of the interpolated precision at num_samples recall levels 0 .. 1: at each level the value at the first rank
        whose recall EXCEEDS the level, 0 where no rank does.  NaN without ground truth (0 with no_gt_is_zero)."""
        if not self.num_gt:
            return self._scalar(0.0 if no_gt_is_zero else float("nan"))
        n = self.recall.numel()
        levels = torch.linspace(0, 1, num_samples, dtype=self.recall.dtype, device=self.recall.device)
        first = torch.searchsorted(self.recall.contiguous(), levels, right=True)      # recall never decreases
        reached = first < n
        values = torch.zeros_like(levels)
        values[reached] = self.precision_interpolated[first[reached]]
        return values.mean()


def average_precision(curve, num_samples=None, no_gt_is_zero=False):
    """num_samples None: the all-points AP of the curve, else the AP sampled at that many recall levels (a 0-d tensor)."""
    if num_samples is None:
        return curve.get_ap_interpolated_all_points(no_gt_is_zero=no_gt_is_zero)
    return curve.get_ap_interpolated_sampled(num_samples=num_samples, no_gt_is_zero=no_gt_is_zero)


# ---- confusion ----------------------------------------------------------------------------------------------------------------
class ConfusionCalculator:
    """evaluation.py:1159-1175: int64 [C, C] counts of pred * C + gt over the rows with 0 <= gt < C (scn_eval_confusion).  The
    reference asserts that every such row's pred is in range; here those rows are counted on the device (`n_bad_pred`, summed
    over the calls) and `check()` -- which the accumulators call when the metrics are read -- raises ScnError."""

    def __init__(self, num_classes):
        if not 1 <= int(num_classes) <= CONFUSION_MAX_CLASSES:
            raise ValueError(f"num_classes must be in 1 .. {CONFUSION_MAX_CLASSES}")
        self.num_classes = int(num_classes)
        self.n_bad_pred = None

    def __call__(self, pred, gt):
        pred, gt = _need_cuda(pred, "pred"), _need_cuda(gt, "gt")
        pred, gt = pred.detach().to(torch.int64).reshape(-1).contiguous(), gt.detach().to(torch.int64).reshape(-1).contiguous()
        if pred.numel() != gt.numel():
            raise L.ScnError(f"{pred.numel()} predictions, {gt.numel()} labels")
        c = self.num_classes
        out = torch.empty((c, c), dtype=torch.int64, device=pred.device)
        bad = torch.empty(1, dtype=torch.int64, device=pred.device)
        L.check(L.lib().scn_eval_confusion(L.ptr(pred), L.ptr(gt), pred.numel(), c, L.ptr(out), L.ptr(bad), L.stream()))
        self.n_bad_pred = bad if self.n_bad_pred is None else self.n_bad_pred + bad
        return out

    def check(self):
        if self.n_bad_pred is not None:
            n = int(self.n_bad_pred.item())
            if n:
                raise L.ScnError(f"ConfusionCalculator: {n} rows with a valid label have a prediction outside "
                                 f"0 .. {self.num_classes - 1}")


class ConfusionAccumulator:
    """evaluation.py:1178-1194; the matrices stay on the device until get_confusion_matrix."""

    def __init__(self, confusion_calculator, device=None):
        self.confusion_calculator = confusion_calculator
        self.confusion_list = []

    def add_batch(self, pred, gt):
        self.confusion_list.append(self.confusion_calculator(pred, gt))

    def add_list_batch(self, pred, gt):
        self.add_batch(torch.cat(list(pred)), torch.cat(list(gt)))

    def get_confusion_matrix(self, device=None):
        if hasattr(self.confusion_calculator, "check"):
            self.confusion_calculator.check()
        return ConfusionMatrix(torch.stack(self.confusion_list).sum(0))


class ConfusionMatrix:
    """Per-class counts and IoU of an int64 [C, C] matrix indexed [prediction, label] (one copy to the host): tp = diagonal,
    fp = row sum - tp, fn = column sum - tp, iou = tp / (tp + fp + fn) as one fp32 division, average_iou = the mean over the
    classes that occur (NaN entries skipped)."""

    def __init__(self, confusion_matrix):
        m = confusion_matrix.cpu().numpy().astype(np.int64)
        predicted, labelled = m.sum(axis=1), m.sum(axis=0)
        self.confusion_matrix = m
        self.tp = np.diagonal(m).copy()
        self.fp, self.fn = predicted - self.tp, labelled - self.tp
        with np.errstate(divide="ignore", invalid="ignore"):
            self.iou = self.tp.astype(np.float32) / (predicted + labelled - self.tp).astype(np.float32)
        self.average_iou = _nanmean(self.iou)


def _nanmean(a):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        return np.nanmean(a)


class BinaryMaskConfusionCalculator:
    """evaluation.py:1120-1127 for all masks of a batch: `batch(pred_list, gt_list)` -> list of int64 [G_s, 2, 2]
    [[tp, fp], [fn, tn]] of prediction i against ground truth i (one scn_eval_mask_iou call); called as the reference calls it
    (one prediction, one ground-truth mask) it returns the [2, 2] of the pair."""

    def __init__(self, mask_threshold):
        self.mask_threshold = mask_threshold

    def batch(self, pred_list, gt_list):
        r = mask_iou(_packed_list(pred_list, "pred", self.mask_threshold), _packed_list(gt_list, "gt"), pair_confusion=True)
        return [r.sample(s)["confusion"] for s in range(len(r.n_pred))]

    def __call__(self, pred, gt_mask, bbox=None):
        _need_cuda(pred, "pred")
        _need_cuda(gt_mask, "gt_mask")
        return self.batch([pred.reshape(1, -1)], [gt_mask.reshape(1, -1)])[0][0]


class BinaryConfusionAccumulator:
    """evaluation.py:1130-1156."""

    def __init__(self, binary_confusion_calculator, device=None):
        self.binary_confusion_calculator = binary_confusion_calculator
        self.confusion_matrix_list, self.label_array_list = [], []

    def add_batch(self, pred_list_list, gt_mask_list_list, bbox_list_list, label_list_list):
        labels = list(label_list_list)
        for i, l in enumerate(labels):
            _need_cuda(l, f"label[{i}]")
        self.confusion_matrix_list += self.binary_confusion_calculator.batch(pred_list_list, gt_mask_list_list)
        self.label_array_list += labels

    def add_sample(self, pred_list, gt_mask_list, bbox_list, label_list):
        self.add_batch([pred_list], [gt_mask_list], [bbox_list], [label_list])

    def get_binary_confusion_matrix_collection(self, classes, device=None):
        dev = self.label_array_list[0].device if self.label_array_list else _device()
        conf = torch.cat(self.confusion_matrix_list) if self.confusion_matrix_list else \
            torch.zeros((0, 2, 2), dtype=torch.int64, device=dev)
        labels = torch.cat(self.label_array_list) if self.label_array_list else torch.zeros(0, dtype=torch.int64, device=dev)
        return BinaryConfusionMatrixCollection(conf, labels, classes)


class BinaryConfusionMatrixCollection:
    """Binary mask confusion [[tp, fp], [fn, tn]] of n instance pairs, grouped by the instance's label (one copy to the host).
    classwise_confusion_matrices int64 [2, 2, C] = the sums per class (classwise_tp / _fp / _fn / _tn its entries);
    classwise_iou = tp / (tp + fp + fn) of those sums; classwise_mean_iou = the mean of the pairs' own IoUs (fp32) per class;
    average_iou / mean_average_iou = their means over the classes that occur."""

    def __init__(self, confusion_tensor, label_array, classes):
        n = int(confusion_tensor.shape[0])
        blob = torch.cat([confusion_tensor.reshape(-1).to(torch.int64), label_array.reshape(-1).to(torch.int64)]).cpu().numpy()
        pairs, labels = blob[:4 * n].reshape(n, 2, 2), blob[4 * n:]
        classes = classes.tolist() if torch.is_tensor(classes) else list(classes)
        sums = np.zeros((2, 2, len(classes)), np.int64)
        mean_iou = np.full(len(classes), np.nan)
        for j, c in enumerate(classes):
            mine = pairs[labels == c]
            sums[:, :, j] = mine.sum(axis=0)
            if len(mine):
                hit, union = mine[:, 0, 0], mine[:, 0, 0] + mine[:, 0, 1] + mine[:, 1, 0]
                with np.errstate(divide="ignore", invalid="ignore"):
                    mean_iou[j] = (hit.astype(np.float32) / union.astype(np.float32)).mean(dtype=np.float32)
        self.classwise_confusion_matrices = sums
        self.classwise_tp, self.classwise_fp, self.classwise_fn, self.classwise_tn = sums[0, 0], sums[0, 1], sums[1, 0], sums[1, 1]
        union = self.classwise_tp + self.classwise_fp + self.classwise_fn
        self.classwise_iou = np.array([t / u if u else float("nan") for t, u in zip(self.classwise_tp, union)], np.float64)
        self.classwise_mean_iou = mean_iou
        self.average_iou, self.mean_average_iou = _nanmean(self.classwise_iou), _nanmean(mean_iou)


# ---- the metric dictionaries --------------------------------------------------------------------------------------------------
class _IndexNames:
    """Default class names: the class index itself."""

    def __getitem__(self, idx):
        return idx


def metric_key(name, metric, threshold, method):
    """The reference's key strings: `mask_AP_0.5`, `bbox_mAP_[0.5:0.95:0.05]`, ...  For a sampled method the reference's
    suffix is the literal text `_{method}_points` (its f-string is not nested): kept, so that its logs and dashboards line up."""
    return f"{name}_{metric}_{threshold}" + ("" if method is None else "_{method}_points")


class EvaluationHelper:
    """Turns accumulators into the reference's two metric dictionaries (its class of the same name, evaluation.py:866).
    overlap_thresholds: numbers, and (label, (numbers...)) tuples whose AP / mAP are averaged under the label;
    overlap_methods: None = all-points AP, an integer = AP sampled at that many recall levels.
    __call__ -> (combined_metrics, single_class_metrics, {}, confusion matrices, overlap confusion matrices, binary
    collections); the reference's raw_pr_curves (third place) are not produced.  Every overlap accumulator waits for the host
    once: all its thresholds and classes are one matching launch."""

    def __init__(self, overlap_thresholds, overlap_class_indices, overlap_class_names=None, overlap_methods=(None, 11),
                 confusion_class_names=None, device=None):
        self.plain_thresholds = [t for t in overlap_thresholds if not isinstance(t, tuple)]
        self.threshold_ranges = [(label, tuple(members)) for label, members in
                                 (t for t in overlap_thresholds if isinstance(t, tuple))]
        every = set(self.plain_thresholds)
        for _, members in self.threshold_ranges:
            every.update(members)
        self.overlap_thresholds = sorted(every)
        self.overlap_methods = list(overlap_methods)
        self.overlap_class_indices = overlap_class_indices
        self.overlap_class_names = overlap_class_names if overlap_class_names is not None else _IndexNames()
        self.confusion_class_names = confusion_class_names if confusion_class_names is not None else _IndexNames()
        self.device = device

    def _overlap_metrics(self, name, accumulator, combined, per_class):
        classes = None
        if accumulator.has_classes():
            classes = [int(c) for c in (self.overlap_class_indices.tolist() if torch.is_tensor(self.overlap_class_indices)
                                        else self.overlap_class_indices)]
        matched = accumulator.matched(self.overlap_thresholds, classes)                 # the one host wait
        for method in self.overlap_methods:
            ap, class_ap = {}, {}
            for t in self.overlap_thresholds:
                ap[t] = average_precision(PrecisionRecallCurve(*matched[(None, float(t))]), method).item()
                if classes is not None:
                    class_ap[t] = np.array([average_precision(PrecisionRecallCurve(*matched[(c, float(t))]), method).item()
                                            for c in classes], np.float32)
            for t in self.plain_thresholds:
                combined[metric_key(name, "AP", t, method)] = ap[t]
            for label, members in self.threshold_ranges:
                combined[metric_key(name, "AP", label, method)] = _nanmean([ap[t] for t in members])
            if classes is None:
                continue
            for t in self.plain_thresholds:
                combined[metric_key(name, "mAP", t, method)] = _nanmean(class_ap[t])
                per_class[metric_key(name, "class_AP", t, method)] = {self.overlap_class_names[i]: v
                                                                      for i, v in enumerate(class_ap[t])}
            for label, members in self.threshold_ranges:
                combined[metric_key(name, "mAP", label, method)] = _nanmean([_nanmean(class_ap[t]) for t in members])

    def __call__(self, overlap_accumulators, confusion_accumulators, overlap_confusion_accumulators,
                 binary_confusion_accumulators):
        combined, per_class = {}, {}
        for name, accumulator in overlap_accumulators.items():
            self._overlap_metrics(name, accumulator, combined, per_class)
        matrices = {}
        for kind, group, names in (("plain", confusion_accumulators, self.confusion_class_names),
                                   ("overlap", overlap_confusion_accumulators, self.overlap_class_names)):
            matrices[kind] = {}
            for name, accumulator in group.items():
                cm = matrices[kind][name] = accumulator.get_confusion_matrix(device=self.device)
                combined[f"{name}_avg_iou"] = cm.average_iou
                per_class[f"{name}_iou"] = {f"{names[i]}": v for i, v in enumerate(cm.iou)}
        binary = {}
        for name, accumulator in binary_confusion_accumulators.items():
            b = binary[name] = accumulator.get_binary_confusion_matrix_collection(self.overlap_class_indices)
            combined[f"{name}_mean_avg_iou"] = b.mean_average_iou
            combined[f"{name}_average_iou"] = b.average_iou
            per_class[f"{name}_iou"] = {f"{self.overlap_class_names[i]}": v for i, v in enumerate(b.classwise_iou)}
        return combined, per_class, {}, matrices["plain"], matrices["overlap"], binary
