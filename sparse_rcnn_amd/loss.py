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
"""
from __future__ import annotations

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
