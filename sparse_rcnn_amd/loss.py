"""The reference's RPN loss on the device (`ndsis.modules.loss`: RpnLoss, BatchwiseBboxTargetSelector; the anchor targets of
`AnchorDescriptionMultiLevel.get_bbox_targets`, ndsis/modules/anchor.py:148-165 -> utils/bbox.py select_bbox + bbox_transform).

    gt boxes (list of [n_i, 2, 3])  --rpn_target_calculator(anchors)-->  max_overlaps [B, N], argmax [B, N], bbox_targets [B, N, 2, 3]
        (scn_rpn_targets: IoU of every inside anchor against every box of its sample, bit-equal to the reference)
    --BatchwiseBboxTargetSelector-->  labels, score_weight, bbox_weights [B, N]
        (scn_rpn_sample_batchwise: counts, draw and weights on the device -- the reference's `torch.nonzero` / `len` host waits
         and numpy draw become a radix select over keyed hashes; the draw is reproducible from (seed, draw counter))
    --RpnLoss-->  rpn_score_loss, rpn_bbox_loss (0-dim)
        (scn_rpn_loss: BCE-with-logits + smooth L1 and both gradients in one pass; backward = one scaling launch)

Nothing on this path waits on the host: no `.item()`, `.cpu()` or `nonzero`.  The targets and the draw depend on the anchors and
the boxes only, so they can be queued before the network that produces rpn_score / rpn_bbox runs (`RpnLoss.prepare`).
Each data-parallel rank normalises over its own samples (the reference's batch is one process).

The mask loss (OverlapCalculator, TrainSelector, MaskLoss: the second half of this file) follows the same rules, and so do the
class and segmentation losses and the container that combines all of them (`Loss`: the end of this file).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib as L

__all__ = ["rpn_target_calculator", "RpnTargetCalculator", "BatchwiseBboxTargetSelector", "SamplewiseBboxTargetSelector",
           "RpnLoss"]


def _device_f32(t, name, dims=None):
    if not torch.is_tensor(t):
        raise ValueError(f"{name}: a tensor is required, got {type(t).__name__}")
    if not t.is_cuda:
        raise L.ScnError(f"{name}: a GPU tensor is required (there is no CPU path)")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: fp32 is required, got {t.dtype}")
    if dims is not None and tuple(t.shape[-len(dims):]) != dims:
        raise ValueError(f"{name}: trailing shape {tuple(dims)} required, got {tuple(t.shape)}")
    return t.contiguous()


class RpnTargetCalculator:
    """`get_bbox_targets(gt_bbox_batch)` of the reference's anchor description over fixed anchors [N, 2, 3] = (centre, size):
    calculator(list of [n_i, 2, 3] (start, stop) boxes) -> (max_overlaps [B, N], argmax [B, N] int64, bbox_targets [B, N, 2, 3])."""

    def __init__(self, anchors):
        self.anchors = _device_f32(anchors, "anchors", (2, 3)).reshape(-1, 2, 3)
        self._gt_cache = None

    def _concat(self, gt_bbox_batch):
        """-> (boxes [total, 2, 3] on the anchors' device, host offsets).  The shapes are host facts: no wait."""
        dev = self.anchors.device
        offs = [0]
        parts = []
        for i, g in enumerate(gt_bbox_batch):
            if not torch.is_tensor(g) or g.dim() != 3 or tuple(g.shape[1:]) != (2, 3):
                raise ValueError(f"gt_bbox[{i}]: [n, 2, 3] (start, stop) boxes required, got "
                                 f"{tuple(g.shape) if torch.is_tensor(g) else type(g).__name__}")
            if g.dtype != torch.float32:
                raise ValueError(f"gt_bbox[{i}]: fp32 is required, got {g.dtype}")
            if g.device != dev:
                raise L.ScnError(f"gt_bbox[{i}] is on {g.device}, the anchors on {dev}")
            offs.append(offs[-1] + g.shape[0])
            parts.append(g.reshape(-1, 6))
        gt = torch.cat(parts, 0).contiguous() if offs[-1] else None
        return gt, offs

    def __call__(self, gt_bbox_batch):
        gt_bbox_batch = list(gt_bbox_batch)
        gt, offs = self._concat(gt_bbox_batch)
        return self.from_concatenated(gt, offs)

    def from_concatenated(self, gt, offs):
        """gt: [total, 6] device boxes of all samples, offs: host list of batch + 1 row offsets."""
        B, N = len(offs) - 1, self.anchors.shape[0]
        dev = self.anchors.device
        ov = torch.empty((B, N), dtype=torch.float32, device=dev)
        am = torch.empty((B, N), dtype=torch.int64, device=dev)
        tg = torch.empty((B, N, 2, 3), dtype=torch.float32, device=dev)
        ho = L.host_i64(B + 1)
        for i, o in enumerate(offs):
            ho[i] = int(o)
        L.check(L.lib().scn_rpn_targets(L.ptr(self.anchors), N, L.ptr(gt), ho, B, L.ptr(ov), L.ptr(am), L.ptr(tg), L.stream()))
        return ov, am, tg

    get_bbox_targets = __call__


def rpn_target_calculator(anchors):
    """The reference's `rpn_target_calculator` (anchor_description.get_bbox_targets) over the inside anchors [N, 2, 3]."""
    return RpnTargetCalculator(anchors)


class BatchwiseBboxTargetSelector(nn.Module):
    """`BatchwiseBboxTargetSelector(positive_overlap, negative_overlap, max_weight)` (loss.py:390-431) on the device.
    forward(overlaps [B, N]) -> (labels, score_weight, bbox_weights), each [B, N] fp32.  Positives: overlap >= positive_overlap,
    negatives: < negative_overlap; all of the smaller set is kept and as many members of the larger set are drawn, uniformly
    without replacement.  The reference draws with numpy's global generator; this draw is a function of (seed, draw counter),
    the counter advancing by one per call (saved in state_dict).  `last_counts`: int64 [2] device tensor (#pos, #neg)."""

    def __init__(self, positive_overlap=0.35, negative_overlap=0.15, max_weight=(1 / 8), seed=0):
        super().__init__()
        if not negative_overlap <= positive_overlap:
            raise ValueError("negative_overlap <= positive_overlap required")
        if not max_weight > 0:
            raise ValueError("max_weight > 0 required")
        self.positive_overlap = positive_overlap
        self.negative_overlap = negative_overlap
        self.min_inverse_weight = 1 / max_weight
        self.seed = int(seed) & (2 ** 64 - 1)
        self.counter = 0
        self._ws = {}
        self.last_counts = None

    def get_extra_state(self):
        return {"seed": self.seed, "counter": self.counter}

    def set_extra_state(self, state):
        self.seed, self.counter = int(state["seed"]), int(state["counter"])

    def _workspace(self, device):
        key = (device.index if device.index is not None else torch.cuda.current_device(), L.stream())
        ws = self._ws.get(key)
        if ws is None:          # zero once; every call leaves it zero (include/scn_mi355x.h)
            ws = self._ws[key] = torch.zeros(L.lib().scn_rpn_sample_workspace_bytes(), dtype=torch.uint8, device=device)
        return ws

    def draw(self, overlaps, counter):
        """The selection for an explicit draw counter (the counter of this module is left alone)."""
        ov = _device_f32(overlaps, "overlaps")
        if ov.dim() < 1:
            raise ValueError("overlaps: [B, N] required")
        n = ov.numel()
        if n >= 2 ** 31:
            raise ValueError("overlaps: fewer than 2^31 entries required")
        labels, sw, bw = (torch.empty_like(ov) for _ in range(3))
        counts = torch.empty(2, dtype=torch.int64, device=ov.device)
        L.check(L.lib().scn_rpn_sample_batchwise(L.ptr(ov), n, float(self.positive_overlap), float(self.negative_overlap),
                                                 float(self.min_inverse_weight), self.seed, int(counter) & (2 ** 64 - 1),
                                                 L.ptr(self._workspace(ov.device)), L.ptr(labels), L.ptr(sw), L.ptr(bw),
                                                 L.ptr(counts), L.stream()))
        self.last_counts = counts
        return labels, sw, bw

    def forward(self, overlaps):
        out = self.draw(overlaps, self.counter)
        self.counter += 1
        return out


class SamplewiseBboxTargetSelector(nn.Module):
    """Not provided: the reference's configuration subsamples batch-wide (`batchwise_subsample=True`, scannet_config/run.py)."""

    def __init__(self, *args, **kwargs):
        raise ValueError("SamplewiseBboxTargetSelector is not provided on the device: use BatchwiseBboxTargetSelector "
                         "(the reference's configuration, batchwise_subsample=True)")


class _RpnLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rpn_score, rpn_bbox, labels, score_weight, bbox_targets, bbox_weights, sigma):
        n = rpn_score.numel()
        dev = rpn_score.device
        score_loss = torch.empty((), dtype=torch.float32, device=dev)
        bbox_loss = torch.empty((), dtype=torch.float32, device=dev)
        dscore = torch.empty_like(rpn_score)
        dbbox = torch.empty_like(rpn_bbox)
        scratch = L.scratch(L.lib().scn_rpn_loss_scratch_bytes(n), dev)
        L.check(L.lib().scn_rpn_loss(L.ptr(rpn_score), L.ptr(rpn_bbox), L.ptr(labels), L.ptr(score_weight), L.ptr(bbox_targets),
                                     L.ptr(bbox_weights), n, float(sigma), L.ptr(scratch), L.ptr(score_loss), L.ptr(bbox_loss),
                                     L.ptr(dscore), L.ptr(dbbox), L.stream()))
        ctx.save_for_backward(dscore, dbbox)
        return score_loss, bbox_loss

    @staticmethod
    def backward(ctx, g_score, g_bbox):
        dscore, dbbox = ctx.saved_tensors
        want_s = g_score is not None and ctx.needs_input_grad[0]
        want_b = g_bbox is not None and ctx.needs_input_grad[1]
        out_s = torch.empty_like(dscore) if want_s else None
        out_b = torch.empty_like(dbbox) if want_b else None
        if want_s or want_b:
            gs = g_score.float().contiguous() if want_s else None
            gb = g_bbox.float().contiguous() if want_b else None
            L.check(L.lib().scn_rpn_loss_scale(L.ptr(dscore), L.ptr(dbbox), dscore.numel(), L.ptr(gs), L.ptr(gb), L.ptr(out_s),
                                               L.ptr(out_b), L.stream()))
        return out_s, out_b, None, None, None, None, None


class RpnLoss(nn.Module):
    """`RpnLoss(bbox_target_selector, sigma)` (loss.py:212-252): forward(gt_bbox, rpn_target_calculator, rpn_score [B, N],
    rpn_bbox [B, N, 2, 3]) -> (rpn_score_loss, rpn_bbox_loss), 0-dim fp32: sum of BCE-with-logits weighted by score_weight,
    sum of smooth L1 (sigma) weighted per anchor by bbox_weights.  The selector must be a BatchwiseBboxTargetSelector (or any
    callable with its contract); `rpn_target_calculator` is `rpn_target_calculator(anchors)`, DenseRpn / MultiLevelRpn
    `.target_calculator(...)` or any callable with get_bbox_targets' contract.
    `prepare(gt_bbox, rpn_target_calculator)` queues targets and draw alone (before the network runs);
    `loss(prepared, rpn_score, rpn_bbox)` finishes.  `last_prepared`: the (overlaps, argmax, targets, labels, score_weight,
    bbox_weights) of the last call."""

    def __init__(self, bbox_target_selector, sigma=2.):
        super().__init__()
        if isinstance(bbox_target_selector, SamplewiseBboxTargetSelector):     # (its constructor refuses already)
            raise ValueError("SamplewiseBboxTargetSelector is not provided")
        self.bbox_target_selector = bbox_target_selector
        self.sigma = float(sigma)
        if not self.sigma > 0:
            raise ValueError("sigma > 0 required")
        self.last_prepared = None

    def prepare(self, gt_bbox, rpn_target_calculator):
        ov, am, tg = rpn_target_calculator(gt_bbox)
        labels, sw, bw = self.bbox_target_selector(ov)
        return ov, am, tg, labels, sw, bw

    def loss(self, prepared, rpn_score, rpn_bbox):
        ov, am, tg, labels, sw, bw = prepared
        self.last_prepared = prepared
        rpn_score = _device_f32(rpn_score, "rpn_score")
        rpn_bbox = _device_f32(rpn_bbox, "rpn_bbox", (2, 3))
        if rpn_score.dim() != 2 or tuple(rpn_bbox.shape) != tuple(rpn_score.shape) + (2, 3):
            raise ValueError(f"rpn_score [B, N] and rpn_bbox [B, N, 2, 3] required, got {tuple(rpn_score.shape)} and "
                             f"{tuple(rpn_bbox.shape)}")
        for name, t, shp in (("labels", labels, rpn_score.shape), ("score_weight", sw, rpn_score.shape),
                             ("bbox_weights", bw, rpn_score.shape), ("bbox_targets", tg, rpn_bbox.shape)):
            t = _device_f32(t, name)
            if t.shape != shp:
                raise ValueError(f"{name}: shape {tuple(shp)} required (the anchors of the targets and of rpn_score differ?), "
                                 f"got {tuple(t.shape)}")
            if t.device != rpn_score.device:
                raise L.ScnError(f"{name} is on {t.device}, rpn_score on {rpn_score.device}")
        return _RpnLossFunction.apply(rpn_score, rpn_bbox, labels.contiguous(), sw.contiguous(), tg.contiguous(),
                                      bw.contiguous(), self.sigma)

    def forward(self, gt_bbox, rpn_target_calculator, rpn_score, rpn_bbox):
        return self.loss(self.prepare(gt_bbox, rpn_target_calculator), rpn_score, rpn_bbox)


# ---- mask loss ----------------------------------------------------------------------------------------------------------
# The reference's mask-training path (ndsis/modules/model.py OverlapCalculator :896-916, TrainSelector :919-1014,
# SparseMaskLossSelector :1152-1227; ndsis/modules/loss.py MaskLoss :271-318) on the device (csrc/scn_maskloss.hip):
#
#     roi boxes, gt boxes  --OverlapCalculator / TrainSelector-->  forward boxes (drawn proposals ++ all gt), gt_association
#         (scn_mask_overlap_draw: IoU, max, argmax and the draw in one launch, one workgroup per sample)
#     --MaskBranch (crop + network)-->  mask_scores [M, K], (RoiSelection, counts, batch_splits)
#     --MaskLoss-->  0-dim loss (scn_mask_loss: per-box BCE in double + one finishing block; backward: one launch)
#
# Nothing here waits on the host: every count the kernels need is a shape (the proposals per sample after RoiSelector.finish,
# the ground truths per sample, the crop's rows), and the tables travel in the kernel arguments.

from collections import namedtuple

SelectionDescriptor = namedtuple("SelectionDescriptor", ["forward_boxes", "pred_selection", "gt_selection", "gt_association"])

__all__ += ["OverlapCalculator", "TrainSelector", "SelectionDescriptor", "PackedMasks", "pack_gt_masks", "MaskLoss"]

MAX_PROPOSALS_PER_SAMPLE = 1024            # csrc/scn_maskloss.hip kMaxProposals


def _boxes_list(boxes, name):
    out = []
    for i, b in enumerate(boxes):
        if not torch.is_tensor(b) or b.dim() != 3 or tuple(b.shape[1:]) != (2, 3):
            raise ValueError(f"{name}[{i}]: [n, 2, 3] (start, stop) boxes required, got "
                             f"{tuple(b.shape) if torch.is_tensor(b) else type(b).__name__}")
        if not b.is_cuda:
            raise L.ScnError(f"{name}[{i}]: a GPU tensor is required (there is no CPU path)")
        if b.dtype != torch.float32:
            raise ValueError(f"{name}[{i}]: fp32 is required, got {b.dtype}")
        out.append(b.detach())
    return out


def _flat(tensors, dtype, device, tail=()):
    """One contiguous tensor over a list: a view when the members already lie back to back in one storage (what
    TrainSelector and SceneStep hand out), else torch.cat (a device copy, no host wait)."""
    n = sum(int(t.shape[0]) for t in tensors)
    if n == 0:
        return torch.empty((0,) + tuple(tail), dtype=dtype, device=device)
    first = tensors[0]
    adjacent = all(t.is_contiguous() and t.dtype == dtype and t.device == first.device for t in tensors)
    if adjacent:                  # (one storage: two allocations may also lie back to back)
        base = first.untyped_storage().data_ptr()
        adjacent = all(t.untyped_storage().data_ptr() == base for t in tensors if t.shape[0])
    if adjacent:
        row = first.element_size() * (first[0].numel() if first.shape[0] else 1)
        ptr = first.data_ptr()
        for t in tensors:
            if t.shape[0] and t.data_ptr() != ptr:
                adjacent = False
                break
            ptr += int(t.shape[0]) * row
    if adjacent and first.shape[0]:
        return first.as_strided((n,) + tuple(first.shape[1:]), first.stride())
    return torch.cat([t.reshape((-1,) + tuple(tail)).to(dtype) for t in tensors], 0).contiguous()


def _offsets(counts):
    ho = L.host_i64(len(counts) + 1)
    acc = 0
    ho[0] = 0
    for i, c in enumerate(counts):
        acc += int(c)
        ho[i + 1] = acc
    return ho


class OverlapCalculator(nn.Module):
    """`OverlapCalculator()` (model.py:896-916): forward(pred_bbox_list, gt_bbox_list) -> [(pred_bbox, gt_bbox, max_overlap,
    argmax_overlap)] per sample; max_overlap fp32 [P_s] and argmax int64 [P_s] (first index of the maximum; 0 and 0 for a
    sample without ground truth).  The IoU is bbox_overlap_prediction's, bit-equal.  One launch for the batch."""

    def forward(self, pred_bbox_list, gt_bbox_list):
        preds = _boxes_list(pred_bbox_list, "pred_bbox")
        gts = _boxes_list(gt_bbox_list, "gt_bbox")
        if len(preds) != len(gts):
            raise ValueError(f"{len(preds)} proposal lists and {len(gts)} ground-truth lists")
        for i, p in enumerate(preds):
            if p.shape[0] > MAX_PROPOSALS_PER_SAMPLE:
                raise ValueError(f"pred_bbox[{i}]: at most {MAX_PROPOSALS_PER_SAMPLE} proposals per sample")
        if not preds:
            return []
        dev = preds[0].device
        pc = [int(p.shape[0]) for p in preds]
        pred = _flat(preds, torch.float32, dev, (2, 3))
        gt = _flat(gts, torch.float32, dev, (2, 3))
        mx = torch.empty(sum(pc), dtype=torch.float32, device=dev)
        am = torch.empty(sum(pc), dtype=torch.int64, device=dev)
        L.check(L.lib().scn_mask_overlap_draw(L.ptr(pred), _offsets(pc), L.ptr(gt), _offsets([g.shape[0] for g in gts]), len(pc),
                                              L.ptr(mx), L.ptr(am), 0, 0.0, 0, 0, 0, None, None, None, None, None, L.stream()))
        out, o = [], 0
        for p, g, n in zip(pred_bbox_list, gt_bbox_list, pc):
            out.append((p, g, mx[o:o + n], am[o:o + n]))
            o += n
        return out


class TrainSelector(nn.Module):
    """`TrainSelector(positive_threshold, negative_threshold=0, random_selector=(24, 0, True))` (model.py:919-1014) as the
    reference's mask network configures it (run.py:799-810): per sample, min(num_pos, #positives) proposals with
    max_overlap >= positive_threshold are drawn uniformly without replacement, and every ground-truth box is appended.

    forward(descriptions) -> (forward_boxes_list, SelectionDescriptor list), descriptions = OverlapCalculator's output.
    Fixed-capacity layout (no count leaves the device): sample s has cap_s = min(num_pos, P_s) slots, then its G_s ground
    truths.  The first min(num_pos, #positives) slots hold the drawn proposals; the others hold the box start = stop = 0,
    which the crop gives no point, with gt_association -1 and pred_selection -1 -- the reference drops such a box's NaN loss,
    so the loss and its gradients are those of the reference's selection.  gt_selection = arange(G_s).
    The draw is a function of (seed, draw counter); the counter advances by one per call and is kept in state_dict
    (as BatchwiseBboxTargetSelector's).  `select(pred_bbox_list, gt_bbox_list)` = OverlapCalculator + forward in one launch.
    `last_drawn`: int64 [batch] device tensor, the proposals drawn per sample."""

    SelectionDescriptor = SelectionDescriptor

    def __init__(self, positive_threshold, negative_threshold=0, random_selector=(24, 0, True), seed=0):
        super().__init__()
        if negative_threshold:
            raise ValueError("TrainSelector: negative_threshold != 0 is not provided (the reference's mask and class paths "
                             "use 0)")
        if random_selector is None:
            raise ValueError("TrainSelector: random_selector=None is not provided (the reference's `all_selector` branch "
                             "raises NameError)")
        if not (isinstance(random_selector, tuple) and len(random_selector) == 3):
            raise ValueError("TrainSelector: random_selector = (num_pos, num_neg, use_gt) required")
        num_pos, num_neg, use_gt = random_selector
        if num_neg:
            raise ValueError("TrainSelector: num_neg != 0 is not provided (no negatives are drawn at negative_threshold 0)")
        if not use_gt:
            raise ValueError("TrainSelector: use_gt=False is not provided (the reference's configuration appends the "
                             "ground truth)")
        if int(num_pos) < 0:
            raise ValueError("TrainSelector: num_pos >= 0 required")
        self.positive_threshold = float(positive_threshold)
        self.negative_threshold = 0
        self.num_pos = int(num_pos)
        self.seed = int(seed) & (2 ** 64 - 1)
        self.counter = 0
        self.last_drawn = None
        self._arange = None

    def get_extra_state(self):
        return {"seed": self.seed, "counter": self.counter}

    def set_extra_state(self, state):
        self.seed, self.counter = int(state["seed"]), int(state["counter"])

    def _gt_range(self, n, dev):
        a = self._arange
        if a is None or a.numel() < n or a.device != dev:
            a = self._arange = torch.arange(max(n, 256), dtype=torch.int64, device=dev)
        return a[:n]

    def _run(self, preds, gts, counter, mx=None, am=None):
        for i, p in enumerate(preds):
            if p.shape[0] > MAX_PROPOSALS_PER_SAMPLE:
                raise ValueError(f"pred_bbox[{i}]: at most {MAX_PROPOSALS_PER_SAMPLE} proposals per sample")
        if len(preds) != len(gts):
            raise ValueError(f"{len(preds)} proposal lists and {len(gts)} ground-truth lists")
        if not preds:
            return [], [], []
        dev = preds[0].device
        pc = [int(p.shape[0]) for p in preds]
        gc = [int(g.shape[0]) for g in gts]
        cap = [min(self.num_pos, n) for n in pc]
        pred = _flat(preds, torch.float32, dev, (2, 3))
        gt = _flat(gts, torch.float32, dev, (2, 3))
        given = mx is not None
        if not given:
            mx = torch.empty(sum(pc), dtype=torch.float32, device=dev)
            am = torch.empty(sum(pc), dtype=torch.int64, device=dev)
        nf = sum(cap) + sum(gc)
        fwd = torch.empty((nf, 2, 3), dtype=torch.float32, device=dev)
        assoc = torch.empty(nf, dtype=torch.int64, device=dev)
        psel = torch.empty(sum(cap), dtype=torch.int64, device=dev)
        drawn = torch.empty(len(pc), dtype=torch.int64, device=dev)
        L.check(L.lib().scn_mask_overlap_draw(L.ptr(pred), _offsets(pc), L.ptr(gt), _offsets(gc), len(pc), L.ptr(mx), L.ptr(am),
                                              1 if given else 0, self.positive_threshold, self.num_pos, self.seed,
                                              int(counter) & (2 ** 64 - 1), _offsets([c + g for c, g in zip(cap, gc)]),
                                              L.ptr(fwd), L.ptr(assoc), L.ptr(psel), L.ptr(drawn), L.stream()))
        self.last_drawn = drawn
        fwd_list, descs, overlaps = [], [], []
        f = o = s = 0
        for p, g, n, c, ng in zip(preds, gts, pc, cap, gc):
            fb = fwd[f:f + c + ng]
            fwd_list.append(fb)
            descs.append(SelectionDescriptor(fb, psel[s:s + c], self._gt_range(ng, dev), assoc[f:f + c + ng]))
            overlaps.append((p, g, mx[o:o + n], am[o:o + n]))
            f, o, s = f + c + ng, o + n, s + c
        return overlaps, fwd_list, descs

    def draw(self, descriptions, counter):
        """forward() for an explicit draw counter (the counter of this module is left alone)."""
        descriptions = list(descriptions)
        preds = _boxes_list([d[0] for d in descriptions], "pred_bbox")
        gts = _boxes_list([d[1] for d in descriptions], "gt_bbox")
        dev = preds[0].device if preds else None
        mx = _flat([_device_f32(d[2], "max_overlap") for d in descriptions], torch.float32, dev)
        am_parts = []
        for i, d in enumerate(descriptions):
            a = d[3]
            if not torch.is_tensor(a) or a.dtype != torch.int64 or not a.is_cuda or a.shape != (preds[i].shape[0],):
                raise ValueError(f"argmax_overlap[{i}]: int64 GPU [P_s] required")
            if d[2].shape != (preds[i].shape[0],):
                raise ValueError(f"max_overlap[{i}]: [P_s] required")
            am_parts.append(a)
        am = _flat(am_parts, torch.int64, dev)
        _, fwd_list, descs = self._run(preds, gts, counter, mx, am)
        return tuple(fwd_list), tuple(descs)

    def forward(self, descriptions):
        out = self.draw(descriptions, self.counter)
        self.counter += 1
        return out

    def select(self, pred_bbox_list, gt_bbox_list):
        """OverlapCalculator and forward in ONE launch: -> (overlap descriptions, forward_boxes_list, descriptors)."""
        out = self._run(_boxes_list(pred_bbox_list, "pred_bbox"), _boxes_list(gt_bbox_list, "gt_bbox"), self.counter)
        self.counter += 1
        return out


class PackedMasks:
    """Ground-truth instance masks packed on the device: `words` int32 (uint32 bit patterns), sample s's [G_s][ceil(N_s / 32)]
    words from `word_offsets[s]`, bit p % 32 of word p / 32 = point row p of the sample.  n_gt / n_points: host lists."""

    def __init__(self, words, n_gt, n_points):
        self.words, self.n_gt, self.n_points = words, list(n_gt), list(n_points)
        self.word_offsets = [0]
        for g, n in zip(self.n_gt, self.n_points):
            self.word_offsets.append(self.word_offsets[-1] + g * ((n + 31) // 32))

    def __len__(self):
        return len(self.n_gt)

    def unpack(self, s):
        """bool device [G_s, N_s] of sample s (for checks)."""
        g, n = self.n_gt[s], self.n_points[s]
        w = (n + 31) // 32
        words = self.words[self.word_offsets[s]:self.word_offsets[s + 1]].view(g, w)
        bits = (words.unsqueeze(-1) >> torch.arange(32, device=words.device, dtype=torch.int32)) & 1
        return bits.reshape(g, w * 32)[:, :n].bool()


def pack_gt_masks(gt_mask_list):
    """list (one per sample) of bool / uint8 [G_s, N_s] masks over the sample's point rows (the reference's batch['gt_mask'])
    -> PackedMasks on the masks' device.  One launch."""
    masks = []
    for i, m in enumerate(gt_mask_list):
        if not torch.is_tensor(m) or m.dim() != 2:
            raise ValueError(f"gt_mask[{i}]: [G, N] required")
        if not m.is_cuda:
            raise L.ScnError(f"gt_mask[{i}]: a GPU tensor is required (there is no CPU path)")
        if m.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"gt_mask[{i}]: bool or uint8 required, got {m.dtype}")
        masks.append(m.contiguous().view(torch.uint8))
    dev = masks[0].device if masks else torch.device("cuda", torch.cuda.current_device())
    n_gt = [int(m.shape[0]) for m in masks]
    n_pt = [int(m.shape[1]) for m in masks]
    out = PackedMasks(None, n_gt, n_pt)
    out.words = torch.empty(max(out.word_offsets[-1], 1), dtype=torch.int32, device=dev)
    B = len(masks)
    if B:
        ptrs = (C.c_void_p * B)(*[m.data_ptr() for m in masks])
        L.check(L.lib().scn_mask_pack(ptrs, (L.i64 * B)(*n_gt), (L.i64 * B)(*n_pt), B,
                                      L.ptr(out.words), L.stream()))
    return out


class _MaskLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, src_row, box_of, assoc, box_offs, labels, gt_offs, packed, pt_offs, class_weights):
        m, k = scores.shape
        n_boxes = int(assoc.shape[0])
        dev = scores.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        scratch = torch.empty(L.lib().scn_mask_loss_scratch_bytes(n_boxes, m), dtype=torch.uint8, device=dev)
        B = len(box_offs) - 1
        L.check(L.lib().scn_mask_loss(L.ptr(scores), m, k, L.ptr(src_row), L.ptr(box_of), L.ptr(assoc), _host(box_offs),
                                      L.ptr(labels), _host(gt_offs), L.ptr(packed.words), _host(packed.word_offsets),
                                      _host(pt_offs), B, L.ptr(class_weights), L.ptr(scratch), L.ptr(loss), L.stream()))
        ctx.save_for_backward(scratch, box_of)
        ctx.dims = (n_boxes, m, k)
        return loss

    @staticmethod
    def backward(ctx, g):
        scratch, box_of = ctx.saved_tensors
        n_boxes, m, k = ctx.dims
        if not ctx.needs_input_grad[0]:
            return (None,) * 10
        d = torch.empty((m, k), dtype=torch.float32, device=scratch.device)
        gg = g.float().contiguous()
        L.check(L.lib().scn_mask_loss_bwd(L.ptr(gg), L.ptr(scratch), n_boxes, m, k, L.ptr(box_of), L.ptr(d), L.stream()))
        return (d,) + (None,) * 9


def _host(offs):
    ho = L.host_i64(len(offs))
    for i, v in enumerate(offs):
        ho[i] = int(v)
    return ho


class MaskLoss(nn.Module):
    """`SparseMaskLossSelector` (the branch with a selection description, model.py:1152-1227) and `MaskLoss(class_weights)`
    (loss.py:271-318) fused: forward(mask_scores [M, K] fp32, selection, descriptions, gt_label, gt_mask) -> 0-dim fp32 loss
    with autograd to mask_scores.  selection = (RoiSelection, box counts per sample, points per sample) as MaskBranch.forward
    returns it; descriptions = TrainSelector's SelectionDescriptor list (gt_association per forward box, -1: no ground
    truth); gt_label = list of int64 [G_s] device tensors; gt_mask = PackedMasks or the list of bool [G_s, N_s] device masks.
    Per box: the logit column of its instance's label, BCE-with-logits against the instance's mask bits, averaged over the
    box's rows; boxes without rows (the reference's NaN) or without ground truth are dropped; the loss is the mean over the
    remaining boxes (with class_weights: sum(w l) / sum(w)), or 0 if none remains."""

    def __init__(self, class_weights=None):
        super().__init__()
        self.class_weights = None if class_weights is None else torch.as_tensor(class_weights, dtype=torch.float32)

    def forward(self, mask_scores, selection, descriptions, gt_label, gt_mask):
        from .roi import RoiSelection, selection_from_matrix
        scores = _device_f32(mask_scores, "mask_scores")
        if scores.dim() != 2:
            raise ValueError(f"mask_scores: [M, K] required, got {tuple(scores.shape)}")
        sel, box_counts, batch_splits = selection
        if not isinstance(sel, RoiSelection):
            sel = selection_from_matrix(sel)
        dev = scores.device
        m, k = scores.shape
        if sel.src_row.shape[0] != m:
            raise L.ScnError(f"mask_scores has {m} rows, the selection {sel.src_row.shape[0]}")
        descriptions, gt_label = list(descriptions), list(gt_label)
        box_counts = [int(c) for c in box_counts]
        splits = [int(c) for c in batch_splits]
        B = len(box_counts)
        if not (len(descriptions) == len(gt_label) == len(splits) == B):
            raise ValueError(f"{B} samples in the selection, {len(descriptions)} descriptions, {len(gt_label)} label lists, "
                             f"{len(splits)} batch splits")
        if sum(box_counts) != sel.n_boxes or sum(splits) != sel.n_points:
            raise L.ScnError("box counts / batch splits do not match the selection")
        assocs = []
        for s, d in enumerate(descriptions):
            a = d.gt_association if hasattr(d, "gt_association") else d[3]
            if not torch.is_tensor(a) or a.dtype != torch.int64 or not a.is_cuda or a.shape != (box_counts[s],):
                raise ValueError(f"descriptions[{s}].gt_association: int64 GPU [{box_counts[s]}] required (one per forward box)")
            assocs.append(a)
        for s, l in enumerate(gt_label):
            if not torch.is_tensor(l) or l.dtype != torch.int64 or not l.is_cuda or l.dim() != 1:
                raise ValueError(f"gt_label[{s}]: int64 GPU [G_s] required")
        if not isinstance(gt_mask, PackedMasks):
            gt_mask = pack_gt_masks(gt_mask)
        if gt_mask.n_gt != [int(l.shape[0]) for l in gt_label] or gt_mask.n_points != splits:
            raise ValueError(f"gt_mask: [G_s, N_s] = {list(zip(gt_mask.n_gt, gt_mask.n_points))} per sample required by the labels "
                             f"and batch splits, {list(zip([int(l.shape[0]) for l in gt_label], splits))}")
        cw = self.class_weights
        if cw is not None:
            if cw.numel() != k:
                raise ValueError(f"class_weights: {k} entries (one per logit column) required, got {cw.numel()}")
            if cw.device != dev:
                cw = self.class_weights = cw.to(dev)
        assoc = _flat(assocs, torch.int64, dev)
        labels = _flat(gt_label, torch.int64, dev)
        box_offs = [0]
        for c in box_counts:
            box_offs.append(box_offs[-1] + c)
        gt_offs = [0]
        for l in gt_label:
            gt_offs.append(gt_offs[-1] + int(l.shape[0]))
        pt_offs = [0]
        for n in splits:
            pt_offs.append(pt_offs[-1] + n)
        return _MaskLossFunction.apply(scores, sel.src_row, sel.box_of, assoc, box_offs, labels, gt_offs, gt_mask, pt_offs, cw)


# ---- class and segmentation losses --------------------------------------------------------------------------------------
# The reference's class path (ndsis/modules/model.py LossFilter / ClassLossSelector :1017-1077, ClassPredictor :785-793,
# SegmentationPredictor :885-893; ndsis/modules/loss.py ClassLoss :255-268 and the segmentation loss :94-97, both
# nn.CrossEntropyLoss(weight, ignore_index=-100, reduction='mean')) on the device (csrc/scn_xent.hip):
#
#     class_scores [BB, C], gt_association  --ClassLossSelector-->  labels (one gather per sample, -100: dropped)
#     --ClassLoss / CrossEntropyLoss-->  0-dim loss (scn_xent_fwd: 2 launches; backward scn_xent_bwd: 1 launch)
#
# Nothing waits on the host: rows are never compacted, a dropped row carries the target `ignore_index` instead.

__all__ += ["CrossEntropyLoss", "ClassLoss", "LossFilter", "ClassLossSelector", "ClassPredictor", "SegmentationPredictor",
            "softmax_argmax"]

MAX_CLASSES = 256                          # csrc/scn_xent.hip kMaxClasses


def _check_logits(logits, name):
    logits = _device_f32(logits, name)
    if logits.dim() != 2:
        raise ValueError(f"{name}: [n, c] required, got {tuple(logits.shape)}")
    if not 1 <= logits.shape[1] <= MAX_CLASSES:
        raise L.ScnError(f"{name}: 1 to {MAX_CLASSES} classes required, got {logits.shape[1]}")
    return logits


class _XentFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, weight, ignore_index, owner):
        n, c = logits.shape
        lib = L.lib()
        # one allocation, kept for backward: [n_bad_targets int64][loss fp32, pad][scratch]
        buf = torch.empty(2 + (lib.scn_xent_scratch_bytes(n, c) + 7) // 8, dtype=torch.int64, device=logits.device)
        base = buf.data_ptr()
        L.check(lib.scn_xent_fwd(logits.data_ptr(), n, c, targets.data_ptr(), L.ptr(weight), ignore_index, base + 16,
                                 base + 8, base, L.stream()))
        owner.n_bad_targets = buf[0]
        ctx.save_for_backward(logits, targets, buf)
        ctx.weight, ctx.ignore_index = weight, ignore_index
        return buf[1:2].view(torch.float32)[0]

    @staticmethod
    def backward(ctx, g):
        logits, targets, buf = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        n, c = logits.shape
        d = torch.empty_like(logits)
        gg = g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous()
        L.check(L.lib().scn_xent_bwd(gg.data_ptr(), logits.data_ptr(), n, c, targets.data_ptr(), L.ptr(ctx.weight),
                                     ctx.ignore_index, buf.data_ptr() + 16, d.data_ptr(), L.stream()))
        return (d,) + (None,) * 4


class CrossEntropyLoss(nn.Module):
    """`nn.CrossEntropyLoss(weight, ignore_index, reduction='mean')` on the device: forward(logits [n, c] fp32, targets [n]
    int64) -> 0-dim fp32 loss = sum_valid w[t] (logsumexp(x) - x[t]) / sum_valid w[t], with autograd to the logits.
    1 <= c <= 256.  A row is valid when its target is in [0, c) and is not `ignore_index`.  A target outside [0, c) that is
    not `ignore_index` (torch: a device assert) drops its row and is counted in `n_bad_targets` (int64 0-dim device tensor,
    the count of the last call).  Without any valid row the loss and the gradient are 0 (torch: NaN): this library's padded
    selector slots make "rows, none valid" its image of the reference's "no box selected", for which ClassLoss returns 0.
    Sums in double in a fixed order: reruns are bitwise identical.  Nothing waits on the host."""

    def __init__(self, weight=None, ignore_index=-100):
        super().__init__()
        self.weight = None if weight is None else torch.as_tensor(weight, dtype=torch.float32).detach().contiguous()
        self.ignore_index = int(ignore_index)
        self.n_bad_targets = None

    def forward(self, logits, targets):
        logits = _check_logits(logits, "logits")
        n, c = logits.shape
        if not torch.is_tensor(targets) or targets.dtype != torch.int64 or targets.shape != (n,):
            raise ValueError(f"targets: int64 [{n}] required")
        if targets.device != logits.device:
            raise L.ScnError(f"targets are on {targets.device}, the logits on {logits.device}")
        w = self.weight
        if w is not None:
            if w.numel() != c:
                raise ValueError(f"weight: {c} entries (one per class) required, got {w.numel()}")
            if w.device != logits.device:
                w = self.weight = w.to(logits.device)
        return _XentFunction.apply(logits, targets.contiguous(), w, self.ignore_index, self)    # (sets self.n_bad_targets)


class ClassLoss(nn.Module):
    """`ClassLoss(class_weights)` (loss.py:255-268): forward(class_output list of [n_s, C], class_target list of [n_s]) ->
    CrossEntropyLoss(class_weights, ignore_index=-100) over the concatenation; 0 without any row."""

    def __init__(self, class_weights=None):
        super().__init__()
        self.loss = CrossEntropyLoss(weight=class_weights, ignore_index=-100)

    @property
    def n_bad_targets(self):
        return self.loss.n_bad_targets

    def forward(self, class_output, class_target):
        class_output, class_target = list(class_output), list(class_target)
        if not class_output:
            raise ValueError("class_output: at least one sample required")
        out = class_output[0] if len(class_output) == 1 else torch.cat(class_output, 0)
        tgt = class_target[0] if len(class_target) == 1 else torch.cat(class_target, 0)
        return self.loss(out, tgt)


class LossFilter(nn.Module):
    """`LossFilter(positive_threshold, negative_threshold=0)` (model.py:1017-1032): forward(max_overlap [P], argmax [P]) ->
    (keep bool [P], gt_association int64 [P]).  keep = overlap >= positive_threshold, or < negative_threshold (then the
    association is -1).  The reference returns the association of the kept rows only; here it keeps the proposals' length
    (no count reaches the host) and the caller gives a dropped row the target `ignore_index`."""

    def __init__(self, positive_threshold, negative_threshold=0):
        super().__init__()
        self.positive_threshold = positive_threshold
        self.negative_threshold = negative_threshold

    def forward(self, max_overlap, argmax_overlap):
        keep = max_overlap >= self.positive_threshold
        assoc = argmax_overlap
        if self.negative_threshold:
            negative = max_overlap < self.negative_threshold
            keep = keep | negative
            assoc = torch.where(negative, torch.full_like(assoc, -1), assoc)
        return keep, assoc


class ClassLossSelector(nn.Module):
    """`ClassLossSelector(positive_threshold, negative_threshold=0, negative_label=-100)` (model.py:1035-1077):
    forward(class_scores [BB, C], selection, descriptions or None, overlap descriptions, gt_labels_list) ->
    (class scores per sample, labels per sample).  With selection descriptions (training) the labels are
    pad(gt_labels, negative_label)[gt_association]; without (the loss over all proposals) the association is LossFilter's.
    Kept rows are NOT compacted: a row the reference would drop keeps its place with the label -100, which ClassLoss
    ignores -- the loss and the gradients are the reference's, and the returned lists have the proposals' length."""

    IGNORE = -100

    def __init__(self, positive_threshold, negative_threshold=0, negative_label=-100):
        super().__init__()
        self.loss_filter = LossFilter(positive_threshold, negative_threshold)
        self.negative_label = negative_label

    def single_sample_selection(self, gt_association, gt_labels):
        padded = nn.functional.pad(gt_labels, (0, 1), value=self.negative_label)
        # -1 reads the pad.  (OverlapCalculator gives argmax 0 to a sample without ground truth, whose overlap 0 is never
        # positive; the clamp keeps that gather, and any other stray association, in bounds without a device assert)
        return padded[gt_association.clamp(-1, gt_labels.shape[0] - 1)]

    def forward(self, class_scores, selection, class_selector_description_list, pred_gt_max_argmax_tuple_list,
                gt_labels_list):
        _, box_sample_count, *_ = selection
        box_sample_count = [int(c) for c in box_sample_count]
        scores = torch.split(class_scores, box_sample_count)
        gt_labels_list = list(gt_labels_list)
        if class_selector_description_list is None:
            labels = []
            for (_, _, mx, am), gl in zip(pred_gt_max_argmax_tuple_list, gt_labels_list):
                keep, assoc = self.loss_filter(mx, am)
                lab = self.single_sample_selection(assoc, gl)
                labels.append(torch.where(keep, lab, torch.full_like(lab, self.IGNORE)))
        else:
            labels = [self.single_sample_selection(d.gt_association if hasattr(d, "gt_association") else d[3], gl)
                      for d, gl in zip(class_selector_description_list, gt_labels_list)]
        for s, (sc, lab) in enumerate(zip(scores, labels)):
            if sc.shape[0] != lab.shape[0]:
                raise ValueError(f"sample {s}: {sc.shape[0]} class scores and {lab.shape[0]} labels")
        return list(scores), labels


def softmax_argmax(logits, probabilities=True):
    """logits [n, c] fp32 -> (indices int64 [n]: the first index of the row's maximum, taken on the logits;
    softmax probabilities fp32 [n, c] or None).  One launch (scn_softmax_argmax); none for n == 0."""
    logits = _check_logits(logits.detach(), "logits")
    n, c = logits.shape
    idx = torch.empty(n, dtype=torch.int64, device=logits.device)
    prob = torch.empty_like(logits) if probabilities else None
    if n:
        L.check(L.lib().scn_softmax_argmax(L.ptr(logits), n, c, L.ptr(prob), L.ptr(idx), L.stream()))
    return idx, prob


class ClassPredictor(nn.Module):
    """`ClassPredictor()` (model.py:785-793): forward(class_predictions [BB, C], selection) -> (class indices per sample,
    class probabilities per sample, class indices [BB])."""

    def forward(self, class_predictions, selection):
        _, box_sample_count, *_ = selection
        counts = [int(c) for c in box_sample_count]
        idx, prob = softmax_argmax(class_predictions)
        return torch.split(idx, counts), torch.split(prob, counts), idx


class SegmentationPredictor(nn.Module):
    """`SegmentationPredictor(sparse=True)` (model.py:885-893): forward(scores [N, C]) -> (class [N], probabilities [N, C])."""

    def __init__(self, sparse=True):
        super().__init__()
        if not sparse:
            raise ValueError("SegmentationPredictor: the dense layout (classes first) is not provided")

    def forward(self, tensor):
        return softmax_argmax(tensor)


# ---- the loss container ---------------------------------------------------------------------------------------------------
# The reference's `Loss` (ndsis/modules/loss.py:12-209): the four criteria above behind one call, their values combined with
# five log-weight parameters (learned with multitask_loss=True; the optimizer's third group, scannet_config/run.py:1441-1444).
#
#     rpn_score_loss, rpn_bbox_loss, class_loss, mask_loss, segmentation_loss (0-dim, on the device; absent ones left out)
#     --scn_loss_combine-->  combined = sum t_i exp(-w_i) + sum w_i, and the 8-float record behind `sublosses`   (1 launch)
#     backward: scn_loss_combine_bwd -> the five term gradients and the five weight gradients                       (1 launch)
#
# The reference reads seven values back per step (`.item()`, loss.py:116-189); here the record stays on the device until a
# value of the mapping is asked for.

import collections.abc

__all__ += ["Loss", "LossCombiner", "LossRecord", "loss_combine", "TERM_NAMES", "WEIGHT_NAMES"]

TERM_NAMES = ("rpn_score", "rpn_bbox", "class", "mask", "segmentation")
# the log-weight parameters in the kernel's order, and the one that scales each term: the reference crosses the two RPN
# weights (loss.py:111-114: rpn_score_loss * exp(-loss_rpn_bbox_weight), rpn_bbox_loss * exp(-loss_rpn_class_weight))
WEIGHT_NAMES = ("loss_rpn_class_weight", "loss_rpn_bbox_weight", "loss_class_weight", "loss_mask_weight",
                "loss_segmentation_weight")
WEIGHT_OF_TERM = (1, 0, 2, 3, 4)
RECORD_NAMES = ("_total_", "_total_multitask_") + TERM_NAMES + ("nan_terms",)

combine_launches = 0                       # scn_loss_combine calls made through loss_combine (tests count them)


def _scalar_f32(t, name):
    if not torch.is_tensor(t):
        raise ValueError(f"{name}: a tensor is required, got {type(t).__name__}")
    if not t.is_cuda:
        raise L.ScnError(f"{name}: a GPU tensor is required (there is no CPU path)")
    if t.dtype != torch.float32 or t.dim() != 0:
        raise ValueError(f"{name}: a 0-dim fp32 tensor is required, got {t.dtype} {tuple(t.shape)}")
    return t


def _pointer_table(tensors):
    return (C.c_void_p * L.LOSS_TERMS)(*[None if t is None else t.data_ptr() for t in tensors])


def loss_combine(terms, log_weights, scale=1.0, root_grad=None, weight_grads=None, running=None):
    """scn_loss_combine (include/scn_mi355x.h): terms = 5 device scalars in TERM_NAMES' order (None: absent), log_weights = 5
    device scalars in WEIGHT_NAMES' order -> the record, fp32 [8] (RECORD_NAMES).  root_grad: fp32 [5] written with
    scale * exp(-w); weight_grads: 5 device scalars (or None entries) that receive += scale * (1 - t exp(-w)); running:
    float64 [9] sums.  One launch, no host wait."""
    global combine_launches
    terms, log_weights = list(terms), list(log_weights)
    if len(terms) != L.LOSS_TERMS or len(log_weights) != L.LOSS_TERMS:
        raise ValueError(f"{L.LOSS_TERMS} terms and {L.LOSS_TERMS} log-weights required")
    for n, t in zip(TERM_NAMES, terms):
        if t is not None:
            _scalar_f32(t, n)
    for n, w in zip(WEIGHT_NAMES, log_weights):
        _scalar_f32(w, n)
    dev = log_weights[0].device
    if root_grad is not None and (root_grad.dtype != torch.float32 or root_grad.numel() < L.LOSS_TERMS or not root_grad.is_cuda
                                  or not root_grad.is_contiguous()):
        raise ValueError(f"root_grad: contiguous fp32 GPU [{L.LOSS_TERMS}] required")
    if running is not None and (running.dtype != torch.float64 or running.numel() < L.LOSS_RECORD + 1 or not running.is_cuda
                                or not running.is_contiguous()):
        raise ValueError(f"running: contiguous float64 GPU [{L.LOSS_RECORD + 1}] required")
    wg = None
    if weight_grads is not None:
        weight_grads = list(weight_grads)
        if len(weight_grads) != L.LOSS_TERMS:
            raise ValueError(f"weight_grads: {L.LOSS_TERMS} entries required")
        for n, g in zip(WEIGHT_NAMES, weight_grads):
            if g is not None:
                _scalar_f32(g, n + " gradient")
        wg = _pointer_table(weight_grads)
    record = torch.empty(L.LOSS_RECORD, dtype=torch.float32, device=dev)
    L.check(L.lib().scn_loss_combine(_pointer_table(terms), _pointer_table(log_weights), float(scale), L.ptr(record),
                                     L.ptr(root_grad), wg, L.ptr(running), L.stream()))
    combine_launches += 1
    return record


class LossRecord(collections.abc.Mapping):
    """The reference's `sublosses` dict over the device record: keys `_total_`, `_total_multitask_` and the present terms in
    the reference's order; the values become Python floats at the first access, through ONE copy of the 8 floats.
    `.tensor`: the device record (RECORD_NAMES); `.isnan`: whether a present term was NaN."""

    def __init__(self, tensor, present):
        self.tensor = tensor
        self._keys = RECORD_NAMES[:2] + tuple(n for n, p in zip(TERM_NAMES, present) if p)
        self._host = None

    def _values(self):
        if self._host is None:
            self._host = self.tensor.tolist()
        return self._host

    def __getitem__(self, key):
        if key not in self._keys:
            raise KeyError(key)
        return self._values()[RECORD_NAMES.index(key)]

    def __iter__(self):
        return iter(self._keys)

    def __len__(self):
        return len(self._keys)

    @property
    def isnan(self):
        return self._values()[L.LOSS_RECORD - 1] > 0

    def __repr__(self):
        return f"LossRecord({dict(self) if self._host is not None else list(self._keys)})"


class _LossCombineFunction(torch.autograd.Function):
    """(owner, t_0 .. t_4 or None, w_0 .. w_4) -> combined.  Backward: one launch, the gradients are views of one buffer."""

    @staticmethod
    def forward(ctx, owner, *tw):
        terms, weights = tw[:L.LOSS_TERMS], tw[L.LOSS_TERMS:]
        record = loss_combine(terms, weights, 1.0, running=owner._running_for(weights[0].device))
        owner._last_record = record
        ctx.present = tuple(t is not None for t in terms)
        ctx.save_for_backward(*[t for t in terms if t is not None], *weights)
        return record[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        weights = saved[len(saved) - L.LOSS_TERMS:]
        it = iter(saved)
        terms = [next(it) if p else None for p in ctx.present]
        gg = g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous()
        buf = torch.empty(2 * L.LOSS_TERMS, dtype=torch.float32, device=gg.device)
        L.check(L.lib().scn_loss_combine_bwd(L.ptr(gg), _pointer_table(terms), _pointer_table(weights), buf.data_ptr(),
                                             buf.data_ptr() + 4 * L.LOSS_TERMS, L.stream()))
        used = [False] * L.LOSS_TERMS
        for i, p in enumerate(ctx.present):
            used[WEIGHT_OF_TERM[i]] = p
        need = ctx.needs_input_grad
        out = [None]
        out += [buf[i] if (ctx.present[i] and need[1 + i]) else None for i in range(L.LOSS_TERMS)]
        out += [buf[L.LOSS_TERMS + j] if (used[j] and need[1 + L.LOSS_TERMS + j]) else None for j in range(L.LOSS_TERMS)]
        return tuple(out)


class LossCombiner(nn.Module):
    """The five log-weight parameters of the reference's `Loss` (`loss_*_weight` = -log(weight), 0-dim fp32, requires_grad =
    multitask_loss; `default_loss`) and the combination of term values with them.  `Loss` adds the criteria; a training step
    that computes its terms itself (trainstep.SceneStep) owns this part alone.  weights: the five `loss_*_weight` values in
    WEIGHT_NAMES' order; has: which of (rpn, class, mask, segmentation) get_weights() reports."""

    def __init__(self, weights=(1, 1, 1, 1, 1), multitask_loss=False, has=(True, True, True, True)):
        super().__init__()
        weights = tuple(weights)
        if len(weights) != L.LOSS_TERMS:
            raise ValueError(f"{L.LOSS_TERMS} weights required")
        for n, v in zip(WEIGHT_NAMES, weights):
            if not (float(v) > 0 and float(v) < float("inf")):
                raise ValueError(f"{n}: a positive finite weight required (its parameter is -log(weight)), got {v}")
        self.multitask_loss = bool(multitask_loss)
        self._has = tuple(bool(h) for h in has)
        self.default_loss = nn.Parameter(torch.zeros([], dtype=torch.float32), requires_grad=False)
        for n, v in zip(WEIGHT_NAMES, weights):
            setattr(self, n, nn.Parameter(-torch.log(torch.tensor(v, dtype=torch.float32)), requires_grad=self.multitask_loss))
        self._running = {}
        self._last_record = None

    def has(self):
        return self._has

    def log_weights(self):
        return [getattr(self, n) for n in WEIGHT_NAMES]

    def _running_for(self, device):
        key = (device.type, device.index)
        buf = self._running.get(key)
        if buf is None:
            buf = self._running[key] = torch.zeros(L.LOSS_RECORD + 1, dtype=torch.float64, device=device)
        return buf

    def combine(self, terms):
        """terms: 5 device scalars in TERM_NAMES' order, None where absent -> (combined_loss, LossRecord)."""
        terms = list(terms)
        combined = _LossCombineFunction.apply(self, *terms, *self.log_weights())
        return combined, LossRecord(self._last_record, [t is not None for t in terms])

    def get_weights(self):
        """The reference's dict (loss.py:193-209), its naming included: `rpn_score` reports exp(-loss_rpn_class_weight)
        although that weight scales the rpn_bbox term.  One copy."""
        w = torch.exp(-torch.stack([p.detach() for p in self.log_weights()])).tolist()
        out = {}
        rpn, cls, mask, seg = self.has()
        if rpn:
            out["rpn_score"], out["rpn_bbox"] = w[0], w[1]
        if cls:
            out["class"] = w[2]
        if mask:
            out["mask"] = w[3]
        if seg:
            out["segment"] = w[4]
        return out

    def running_means(self):
        """Means of the record's entries (RECORD_NAMES; an absent term counts as 0) over the calls since reset_running(), and
        `steps`, their number.  One copy per device the container ran on; {} before the first call."""
        sums = None
        for buf in self._running.values():
            v = buf.tolist()
            sums = v if sums is None else [a + b for a, b in zip(sums, v)]
        if not sums or not sums[-1]:
            return {}
        out = {n: s / sums[-1] for n, s in zip(RECORD_NAMES, sums)}
        out["steps"] = int(sums[-1])
        return out

    def reset_running(self):
        for buf in self._running.values():
            buf.zero_()


class Loss(LossCombiner):
    """`Loss(...)` of the reference (loss.py:12-209) with its signature and defaults: the criteria of this module behind one
    call -- RpnLoss(BatchwiseBboxTargetSelector(**bbox_target_selector_kwargs), sigma), ClassLossSelector + ClassLoss,
    MaskLoss (selector and loss fused), CrossEntropyLoss(segmentation_weights, ignore_index=-100), each built only when its
    `calc_*` flag is on -- and the five parameters `loss_*_weight` = -log(weight), 0-dim fp32, learned when multitask_loss.
    `default_loss` is kept, so the reference's state_dict keys map one to one.  seed: the selector's draw.

    forward(batch, outputs) -> (combined_loss, sublosses) with the reference's keys (`gt_bbox`, `gt_label`, `gt_mask`,
    `gt_segmentation`; `rpn_score`, `rpn_bbox`, `rpn_target_calculator`, `mpn_class`, `mpn_mask`, `spn_segmentation`,
    `is_training`, `mpn_{class,mask}_coord_selection`, `mpn_{class,mask}_box_selection`, `roi_bbox`) and presence rules
    (loss.py:106-171).  `mpn_*_coord_selection` is the branch's selection (RoiSelection, counts, splits) and
    `mpn_*_box_selection` the TrainSelector's descriptors, as this package's MaskBranch / ClassBranch return them.
    combined_loss: 0-dim device tensor, one autograd node over scn_loss_combine / scn_loss_combine_bwd (differentiable once);
    sublosses: a LossRecord.  Nothing waits on the host.
    The `len(...)` presence checks: the reference's `len(selected_class_pred)` / `len(selected_mask_pred)` count per-sample
    lists, so they hold for any batch with a sample.  The class check here counts the same lists.  The mask check counts the
    ROWS of `mpn_mask` (selector and loss are one module here): a batch whose mask rows exist but hold no positive is present
    on both sides -- the criterion returns 0 (no valid row), the term is reported as 0, and its log-weight is still added to
    `_total_multitask_` and gets the gradient 1 -- while a crop without any row makes the mask term ABSENT here, where the
    reference reports 0 and adds the weight.

    Refused (ValueError): calc_bbox with batchwise_subsample=False, sparse=False with calc_mask, a dtype other than fp32."""

    def __init__(self, sigma=2., class_target_overlap_threshold=0.15, batchwise_subsample=False, class_weights=None,
                 mask_class_weights=None, class_class_weights=None, segmentation_weights=None, sparse=False,
                 loss_rpn_class_weight=1, loss_rpn_bbox_weight=1, loss_class_weight=1, loss_mask_weight=1,
                 loss_segmentation_weight=1, multitask_loss=False, dtype=torch.get_default_dtype(), *, calc_bbox, calc_class,
                 calc_mask, calc_segmentation, mask_positive_threshold, class_positive_threshold, class_negative_threshold,
                 class_negative_label, seed=0, **bbox_target_selector_kwargs):
        if dtype != torch.float32:
            raise ValueError(f"Loss: dtype torch.float32 required (the criteria and the combining kernel are fp32), got {dtype}")
        if calc_bbox and not batchwise_subsample:
            raise ValueError("Loss: calc_bbox=True with batchwise_subsample=False (the reference's default) needs "
                             "SamplewiseBboxTargetSelector, which is not provided on the device: pass batchwise_subsample=True, "
                             "as the reference's committed configuration does (scannet_config/run.py)")
        if calc_mask and not sparse:
            raise ValueError("Loss: calc_mask=True with sparse=False needs DenseMaskLossSelector, which is not provided: the "
                             "mask loss here is the sparse one (sparse=True)")
        super().__init__((loss_rpn_class_weight, loss_rpn_bbox_weight, loss_class_weight, loss_mask_weight,
                          loss_segmentation_weight), multitask_loss)
        self.rpn_loss = (RpnLoss(BatchwiseBboxTargetSelector(seed=seed, **bbox_target_selector_kwargs), sigma)
                         if calc_bbox else None)
        self.overlap_calculator = OverlapCalculator() if (calc_class or calc_mask) else None
        if calc_class:
            self.class_loss_selector = ClassLossSelector(class_positive_threshold, class_negative_threshold,
                                                         class_negative_label)
            self.class_loss = ClassLoss(class_weights=class_class_weights)
        else:
            self.class_loss_selector = self.class_loss = None
        self.mask_positive_threshold = mask_positive_threshold
        self.mask_loss = MaskLoss(class_weights=mask_class_weights) if calc_mask else None
        self.segmentation_loss = (CrossEntropyLoss(weight=segmentation_weights, ignore_index=-100)
                                  if calc_segmentation else None)

    def has(self):
        return (self.rpn_loss is not None, self.class_loss is not None, self.mask_loss is not None,
                self.segmentation_loss is not None)

    def forward(self, batch, outputs):
        terms = [None] * L.LOSS_TERMS
        if "rpn_score" in outputs and "rpn_bbox" in outputs and self.rpn_loss is not None:
            terms[0], terms[1] = self.rpn_loss(batch["gt_bbox"], outputs["rpn_target_calculator"], outputs["rpn_score"],
                                               outputs["rpn_bbox"])
        want_class = "mpn_class" in outputs and self.class_loss is not None
        want_mask = "mpn_mask" in outputs and self.mask_loss is not None
        overlaps = None
        if (want_class or want_mask) and not outputs["is_training"]:
            overlaps = self.overlap_calculator(outputs["roi_bbox"], batch["gt_bbox"])
        if want_class:
            pred, gts = self.class_loss_selector(outputs["mpn_class"], outputs["mpn_class_coord_selection"],
                                                 outputs["mpn_class_box_selection"], overlaps, batch["gt_label"])
            if len(pred):
                terms[2] = self.class_loss(pred, gts)
        if want_mask:
            descs = outputs["mpn_mask_box_selection"]
            if descs is None:          # the loss over all proposals: LossFilter(mask_positive_threshold)'s association
                descs = [(None, None, None, torch.where(mx >= self.mask_positive_threshold, am, torch.full_like(am, -1)))
                         for _, _, mx, am in overlaps]
            if len(outputs["mpn_mask"]):
                terms[3] = self.mask_loss(outputs["mpn_mask"], outputs["mpn_mask_coord_selection"], descs, batch["gt_label"],
                                          batch["gt_mask"])
        if "spn_segmentation" in outputs and self.segmentation_loss is not None:
            terms[4] = self.segmentation_loss(outputs["spn_segmentation"], batch["gt_segmentation"])
        return self.combine(terms)

    # -- checkpoints ----------------------------------------------------------------------------------------------------
    def load_reference_state_dict(self, state_dict, prefix="", strict=True):
        """Load the reference `Loss`'s part of a checkpoint: `default_loss` and the five `loss_*_weight`; the criteria's class
        weights (`mask_loss.class_weights`, `class_loss.loss.weight`, `segmentation_loss.weight`) where this container has the
        criterion; `mask_loss.default_loss` is the reference MaskLoss's constant 0.
        -> (missing reference keys, unused checkpoint keys under the prefix)."""
        own = ("default_loss",) + WEIGHT_NAMES
        used, missing = set(), []
        with torch.no_grad():
            for n in own:
                v = state_dict.get(prefix + n)
                if v is None:
                    missing.append(n)
                    continue
                if tuple(v.shape) != ():
                    raise ValueError(f"{prefix + n}: a 0-dim value required, got {tuple(v.shape)}")
                getattr(self, n).copy_(v.to(torch.float32))
                used.add(prefix + n)
            for key, crit in (("mask_loss.class_weights", self.mask_loss),
                              ("class_loss.loss.weight", self.class_loss.loss if self.class_loss is not None else None),
                              ("segmentation_loss.weight", self.segmentation_loss)):
                v = state_dict.get(prefix + key)
                if v is not None and crit is not None:
                    w = v.detach().to(torch.float32).contiguous()
                    if isinstance(crit, MaskLoss):
                        crit.class_weights = w
                    else:
                        crit.weight = w
                    used.add(prefix + key)
            if prefix + "mask_loss.default_loss" in state_dict and self.mask_loss is not None:
                used.add(prefix + "mask_loss.default_loss")
        unused = [k for k in state_dict if k.startswith(prefix) and k not in used]
        if strict and (missing or unused):
            raise KeyError(f"Loss.load_reference_state_dict: missing {missing}, unused {unused}")
        return missing, unused
