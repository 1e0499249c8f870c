"""One data-parallel training step of the sparse path on one rank: what ``bench.py`` times and the at-size parity tests
check.  A step = index build (InputLayer rules + every rulebook; rebuilt per batch as in the reference) + forward +
backward to every parameter and the input features + all-reduce of the flat gradient buffer (RCCL / gloo, N > 1) + SGD
(or, `optimizer="adam"`, the reference's Adam: optim.FlatAdam).

Workloads (BASELINE.json configs; SURVEY.md §8d synthetic inputs):
  cfg2  configs[1]  one ~150k-voxel scene, U-Net backbone 32-64-128-256
  cfg3  configs[2] WITHOUT its RPN ("crop + mask branch only"): cfg2 + 64 synthetic boxes per scene, known before the
                    forward -> sparse ROI crop -> mask branch (maskhead.MaskBranch)
  cfg3-rpn  configs[2] with the RPN boundary INSIDE the step: backbone -> SparseToDense of the anchor level -> dense dilation
                    stack + 1x1 heads (rpn.DenseRpn: by default on THIS library's tile kernels, engine "tiles" -- a dense
                    same-convolution is a submanifold convolution on a fully active grid) -> anchors that leave the scene
                    dropped (anchor.py:103-113) -> RoiSelector (top-k + one-launch NMS) -> <= 64 boxes per scene -> sparse ROI
                    crop -> mask branch -> backward through both (rpn.py; model.py:116-240, anchor_network.py:73-124,
                    proposal_selector.py:23-89).  The boxes exist only after the heads have produced them.  Its RPN is a
                    STAND-IN, lighter than the reference's: ONE anchor level with a 2 x 32 dilation stack and 64 proposals
                    kept (BASELINE configs[2]: "~64 proposals/scene"), where scannet_config/run.py:339,525-536,609,847-853
                    builds two anchor levels with 5 x 128 / 5 x 256 stacks and keeps 256 -- `ref-crop-rpn` has that shape.
  ref-crop-rpn  the reference's own detection step as far as this path reaches: plan 32-48-64-80-96-112 on its training batch
                    (12 crops of 128 x 128 x 64, run.py:364,485-488), SparseToDense of BOTH anchor levels (stride 4: 64 ch,
                    stride 8: 80 ch), a 5 x 128 and a 5 x 256 dilation stack (run.py:525-536,609), 3 + 11 anchors per cell
                    (scannet_config/network.py:7-45) behind 1x1 heads -- or, `upsample_heads=True`, behind the reference's
                    committed heads (run.py:339,532-537: AnchorNetworkUpsample, one transposed convolution per group of
                    anchors on a grid finer than the level's: 182 272 anchors per crop in 11 groups, 88 536 of them inside,
                    where the 1x1 heads have 71 680; rpn.AnchorNetworkUpsample, scn_anchor_up.hip) --, inside-the-scene
                    anchors only, top-1024 / NMS 0.5 / 256 kept (run.py:847-853), boxes clipped to the scene
                    (anchor.py:218-225), sparse ROI crop + mask branch.
  cfg5  configs[4]  one ~600k-voxel scene, 5-level U-Net to 512 channels
configs[3] (8 scenes data-parallel) is cfg3 with one scene per rank.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .dp import FlatParams, broadcast_params, broadcast_tensors
from .maskhead import MaskBranch
from .synthetic import make_batch, make_boxes, make_instances, make_segmentation
from .unet import Backbone

PARTS = ("backbone", "rpn", "class", "mask", "segmentation")      # what SceneStep(train=...) names: the sub-modules of its model
REF_PLAN = (32, 48, 64, 80, 96, 112)      # the reference's own sparse U-Net plan, `arange * 16 + 32` (scannet_config/run.py:539-549,587-591)

WORKLOADS = {      # name -> (channels, grid, active voxels per sample, boxes per scene, BASELINE.json entry, samples per rank)
    "cfg2": ((32, 64, 128, 256), (512, 512, 256), 150_000, 0, "configs[1]", 1),
    # cfg2 with BatchNormReLU in place of every ReLU of the residual units (north_star names the operator; the reference ships it
    # off, run.py:612 `batchnorm=False`): the layer-by-layer path by default (step-executor stages: `bn_stages=True`), two more passes
    # over every slab and direction; under DP each rank normalises with its own scene unless modules._BatchNorm.SYNC is set
    "cfg2-bn": ((32, 64, 128, 256), (512, 512, 256), 150_000, 0, "configs[1] with BatchNormReLU units (batchnorm=True)", 1),
    "cfg3": ((32, 64, 128, 256), (512, 512, 256), 150_000, 64, "configs[2]", 1),
    "cfg3-rpn": ((32, 64, 128, 256), (512, 512, 256), 150_000, 64, "configs[2] with the RPN boundary inside the step", 1),
    "cfg5": ((32, 64, 128, 256, 512), (1024, 1024, 512), 600_000, 0, "configs[4] shape (one scene per GPU)", 1),
    # the network the reference actually trains: 6 levels 32-48-64-80-96-112 ...
    "ref": (REF_PLAN, (512, 512, 256), 150_000, 0, "configs[1] scene, the REFERENCE's own channel plan 32-48-64-80-96-112", 1),
    # ... on its own training input: 12 random crops of 128 x 128 x 64 voxels per batch (run.py:364,485-488)
    "ref-crop": (REF_PLAN, (128, 128, 64), 12_500, 0, "the reference's training batch: 12 crops of 128x128x64 voxels, "
                 "plan 32-48-64-80-96-112", 12),
    "ref-crop-rpn": (REF_PLAN, (128, 128, 64), 12_500, 256, "the reference's training batch (12 crops of 128x128x64, plan "
                     "32-48-64-80-96-112) with its RPN shape: two anchor levels, 5x128 / 5x256 dilation stacks, 256 kept", 12),
}


import os as _os

# developer switch (A/B in tools/): start the ROI batch's index build before the backbone forward (helper thread + stream)
EARLY_ROI_CUT = _os.environ.get("SCN_ROI_EARLY", "0") != "0"
# developer switches (A/B): the RPN's kernels between encoder and decoder; the prefetch thread started after the forward's kernels
RPN_BEFORE_DECODER = _os.environ.get("SCN_RPN_EARLY", "1") != "0"
# (in-process A/B, profiles/r5_ab_index_interference.txt: cfg 2 fp32 5.539 -> 5.512 ms, bf16 3.128 -> 3.094, cfg 3 neutral:
#  starting a thread costs the host ~0.1 ms exactly where the GPU's queue is shallowest, the step boundary)
LATE_PREFETCH = _os.environ.get("SCN_LATE_PREFETCH", "1") != "0"
# backward on the calling thread (torch.autograd.set_multithreading_enabled(False)): no hand-off to the device thread per step
# (A/B inside one process, profiles/r5_ab_inproc.txt: cfg 3 bf16 7.13 -> 6.51 ms per step, cfg 2 bf16 3.44 -> 3.31, fp32 neutral)
BACKWARD_INLINE = _os.environ.get("SCN_BACKWARD_INLINE", "1") != "0"


def _backward(roots, grads, step_scope=False):
    """step_scope: inside executor.step_weight_gradients -- the weight gradients of the compiled stages run as one grid per
    kernel variant after the last backward pass and arrive in `.grad` when the call returns."""
    if step_scope:
        from . import executor
        with executor.step_weight_gradients():
            return _backward(roots, grads)
    if BACKWARD_INLINE:
        with torch.autograd.set_multithreading_enabled(False):
            torch.autograd.backward(roots, grads)
    else:
        torch.autograd.backward(roots, grads)


# the loss container's term slots, in the order of the library's LOSS_TERMS (loss.loss_combine)
TERM_RPN_SCORE, TERM_RPN_BBOX, TERM_CLASS, TERM_MASK, TERM_SEGMENTATION = range(L.LOSS_TERMS)


class _RootLedger:
    """What one micro-batch hands to backward, filled by the parts of `forward_backward` in the order they run: the roots, the
    gradient each is back-propagated with, and -- for the roots that are loss values -- the loss container's view of them:
    `terms[i]` the value of term i (None: not computed), `term_pos[i]` its position among the roots."""
    __slots__ = ("roots", "grads", "terms", "term_pos")

    def __init__(self):
        self.roots, self.grads = [], []
        self.terms, self.term_pos = [None] * L.LOSS_TERMS, {}

    def add(self, value, grad, term=None):
        """grad=None (a loss nothing trainable lies under): the container records the term, backward gets no root."""
        if term is not None:
            self.terms[term] = value
            if grad is None:
                return
            self.term_pos[term] = len(self.roots)
        self.roots.append(value)
        self.grads.append(grad)


class SparseStepModel(torch.nn.Module):
    """Backbone (+ mask branch for cfg3) as one module, so that one flat parameter buffer covers the step."""

    def __init__(self, channels, with_mask, storage, with_rpn=False, n_boxes=64, batchnorm=False, with_class=False,
                 with_segmentation=False, upsample_heads=False, class_storage=None, simple_class=False, bottleneck_divisor=0,
                 main_path_relu=False, relu_first=True, drop_input_relu=True, use_residuals=True, bn_stages=False):
        """bn_stages (with batchnorm; False: nothing changes): the batch-norm backbone runs as step-executor stages
        (unet.SparseUNet).
        bottleneck_divisor, main_path_relu (0 / False: nothing changes): the form of the BACKBONE's residual units
        (unet.residual_block; the reference's switches of the same names, run.py:516-518).  The mask branch's own networks keep
        the plain unit: its level 0 runs on channel-padded slabs, which the other forms do not take.
        relu_first, drop_input_relu, use_residuals (True: nothing changes): the backbone's post-activation units, the ReLU of
        its input stages and its plain convolution blocks (unet.py header; run.py:519 and the defaults of model.py:262-269).
        simple_class (with_class="dense" only; False: nothing changes): the dense arm's head is the reference's class network
        WITHOUT pooling (classhead.ReshapeClassBranch; `simple_class`, run.py:706-710) on the same kept volume, fp32.
        class_storage (with_class="dense" on bf16 storage only; None: nothing changes): "bf16" builds the dense class branch
        with storage=torch.bfloat16 and hands it the RPN's volume in its stored dtype (`rpn.volume_stored`).
        upsample_heads (with_rpn="reference" only; False: nothing changes): the reference's committed RPN heads,
        rpn.AnchorNetworkUpsample with its extra strides and anchor groups, in place of the 1x1 heads.  On bf16-stored
        level tensors the stacks' last ReLU runs on the bf16 slab and the heads read its result widened (fp32 row GEMM, P and scatter).
        with_rpn: False | "stand-in" (cfg3-rpn: one anchor level, 2 x 32 stack) | "reference" (ref-crop-rpn: the reference's two
        anchor levels with 5 x 128 / 5 x 256 stacks, rpn.MultiLevelRpn).
        with_class: the reference's class branch (classhead.ClassBranch) on the coarsest RPN level of the encoder -- the
        reference's `class_output_index=-1` on a main network that ends at its last anchor level (run.py:581-584, 605-608).
        with_class="dense": the reference's DENSE class branch (classhead.DenseClassBranch; run.py:340 `dense_class = True`)
        on the dense volume the RPN's dilation stack of anchor level 0 produces (`class_output_anchor`, run.py:603-607): the RPN
        keeps that volume (keep_volume) and the class loss's gradient reaches the stack.
        with_segmentation: the reference's segmentation head (classhead.SegmentationHead, 20 classes) on the backbone output.
        Both are constructed AFTER the other modules: under one seed the others start from the same values with or without."""
        super().__init__()
        self.backbone = Backbone(7, channels, batchnorm=batchnorm, bf16_blocks=storage, bottleneck_divisor=bottleneck_divisor,
                                 main_path_relu=main_path_relu, relu_first=relu_first, drop_input_relu=drop_input_relu,
                                 use_residuals=use_residuals, bn_stages=bool(bn_stages))
        self.mask = MaskBranch(channels[0], 7, bf16_blocks=storage) if with_mask else None
        self.rpn = self.roi_selector = self.rpn_levels = None      # (rpn_levels: indices of the encoder levels the RPN reads)
        if class_storage not in (None, "bf16"):
            raise ValueError("class_storage: None | 'bf16'")
        if class_storage and (with_class != "dense" or storage != "all"):
            raise ValueError("class_storage='bf16' stores the DENSE class branch's slabs in bf16: it needs the dense arm "
                             "(dense_class=True) on bf16 storage (dtype='bf16')")
        self.class_storage = class_storage
        if simple_class and with_class != "dense":
            raise ValueError("simple_class=True is a head of the dense arm: it needs dense_class=True")
        if simple_class and class_storage:
            raise ValueError("simple_class=True computes in fp32 (it widens a bf16 volume on entry): class_storage='bf16' "
                             "belongs to DenseClassBranch")
        if upsample_heads and with_rpn != "reference":
            raise ValueError("upsample_heads=True needs with_rpn='reference' (the reference's two anchor levels)")
        if with_rpn:
            self._build_rpn(channels, with_rpn, bool(storage), n_boxes, upsample_heads, keep_volume=with_class == "dense")
        self.class_branch = self.segmentation = self.class_level = None
        if with_class:
            if self.rpn is None:
                raise ValueError("with_class needs an RPN (the class branch reads its coarsest level)")
            from .classhead import ClassBranch, DenseClassBranch, ReshapeClassBranch
            if with_class == "dense":
                src = self.rpn.levels[self.rpn.class_output_index] if hasattr(self.rpn, "levels") else self.rpn
                self.class_level = self.rpn_levels[self.rpn.class_output_index if hasattr(self.rpn, "levels") else 0]
                if simple_class:
                    self.class_branch = ReshapeClassBranch(src.width, src.stride)
                else:
                    self.class_branch = DenseClassBranch(src.width, src.stride,
                                                         storage=torch.bfloat16 if class_storage else torch.float32)
            else:
                self.class_level = self.rpn_levels[-1]
                self.class_branch = ClassBranch(channels[self.class_level], 2 ** self.class_level)
        if with_segmentation:
            from .classhead import SegmentationHead
            self.segmentation = SegmentationHead(channels[0], 20)

    def _build_rpn(self, channels, kind, autocast_bf16, n_boxes, upsample_heads, keep_volume):
        """The RPN of `kind` and its selector: which encoder levels it reads, (channels, stride, stack width, anchors) of each."""
        from . import rpn as R
        if kind == "reference":
            # run.py:525-549: anchor paths on the two levels behind the in-between downsamplers (64 ch at stride 4, 80 ch at
            # stride 8 in the plan 32-48-64-80-96-112), anchor_output_channels = [128, 256], num_dilations = 5 (run.py:609);
            # upsample_heads: the anchors of the committed heads and their extra strides (run.py:339,532-537)
            anchors = R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS if upsample_heads else R.REF_ANCHOR_LEVELS_VOXELS
            self.rpn_levels = (2, 3)
            self.rpn = R.MultiLevelRpn([(channels[i], 2 ** i, width, a) for i, width, a in zip(self.rpn_levels, (128, 256), anchors)],
                                       num_dilations=5, autocast_bf16=autocast_bf16, keep_volume=keep_volume,
                                       extra_stride_levels=R.REF_EXTRA_STRIDE_LEVELS if upsample_heads else None)
        else:                        # one anchor path on the coarsest level (run.py:524: num_anchor_pathes = 1), stride 2^(L-1)
            self.rpn_levels = (len(channels) - 1,)
            self.rpn = R.DenseRpn(channels[-1], stride=2 ** (len(channels) - 1), autocast_bf16=autocast_bf16, keep_volume=keep_volume)
        # run.py:847-853: 1024 / 256 / 0.5 (the stand-in: run.py:848-850 with ~64 proposals kept per scene)
        self.roi_selector = R.RoiSelector(1024, n_boxes, 0.5)

    def run_rpn(self, interims):
        lv = [interims[i] for i in self.rpn_levels]
        return self.rpn(lv if len(lv) > 1 else lv[0])

    def run_class(self, interims, boxes):
        """The class branch on `boxes`: the sparse arm reads the encoder level, the dense arm the volume the RPN kept in the
        same forward (run_rpn comes first)."""
        from .classhead import DenseClassBranch, ReshapeClassBranch
        if isinstance(self.class_branch, (DenseClassBranch, ReshapeClassBranch)):
            if self.rpn.volume is None:
                raise L.ScnError("the dense class branch reads the RPN's kept volume: run_rpn first")
            slab, size, batch, md = self.rpn.volume_stored if self.class_storage else self.rpn.volume
            return self.class_branch(slab, size, batch, boxes, metadata=md)
        return self.class_branch(interims[self.class_level], boxes)


class SceneStep:
    def __init__(self, workload="cfg2", device=None, dtype="f32", prefetch=True, seed=1, grad_seed=100, n_buckets=4,
                 target=None, channels=None, grid=None, n_boxes=None, lr=None, weighting="equal", batches_per_step=1,
                 optimizer="sgd", betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, rpn_loss=False, mask_loss=False, n_gt=None,
                 class_loss=False, segmentation_loss=False, batches=None, step_group=True, dense_class=False,
                 upsample_heads=False, class_storage=None, simple_class=False, multitask_loss=False, loss_weights=None,
                 bottleneck_divisor=0, main_path_relu=False, relu_first=True, drop_input_relu=True, use_residuals=True,
                 bn_stages=False, train=None, init_state=None, max_grad_norm=None):
        """max_grad_norm (None: nothing changes -- nothing is built or launched): a positive finite bound on the L2 norm of the
        gradient the update reads -- the mean over ranks and micro-batches -- clipped on the device once per optimizer step, after
        the last micro-batch and the reduction, before Adam or SGD (FlatParams.clip_grad_norm: SCN_OP_GRAD_NORM +
        SCN_OP_GRAD_SCALE, torch.nn.utils.clip_grad_norm_'s arithmetic with the sum of squares in double; no host wait).
        `.grad_norm`: (total_norm, clip_coef, nonfinite) of the last step, read from the device when asked for.  Zero, negative,
        NaN, inf, or a `train=` step whose trained parts have no parameters: ValueError.
        train (None: nothing changes -- every parameter is trained): a non-empty tuple of part names out of `PARTS`
        ("backbone", "rpn", "class", "mask", "segmentation"); the parameters of every part NOT named are frozen
        (requires_grad False) before the flat buffer is built, so the flat buffer, the gradient buckets and the optimizer cover
        the named parts only and a frozen parameter never receives a `.grad` -- the reference's training in stages:
        `mask_only` (run.py:332,1420-1427: train=("mask",)) and `unet_tweak` (run.py:1414-1418: every part but "backbone").  A
        requested loss is computed only if its gradient reaches a trainable parameter (the reference's `calc_* and not
        mask_only`, run.py:891-893): the RPN loss with rpn or backbone trainable, the class loss with class or backbone (with
        dense_class also rpn), the mask loss with mask or backbone, the segmentation loss with segmentation or backbone.  A loss
        that is not computed queues no targets, draws or selector launches, its head is not run in forward_backward (predict()
        and evaluate() still run it) and its attribute (`.rpn_losses`, ...) stays None; a root that requires no gradient gets no
        synthetic gradient either.  The input features require a gradient only with "backbone" trainable: otherwise `.fin.grad`
        stays None and the frozen parts run the executor's forward-only slab plan.  A name that is unknown or names a part the
        step does not have, an empty tuple, or multitask_loss=True beside it: ValueError.  With more than one rank the frozen
        parameters are broadcast once at construction.  `loss_weights` may name every requested loss; the container combines
        the computed ones.
        init_state (None: nothing changes): a `state_dict` of an earlier step's `.model`, the hand-over between stages, applied
        before the flat buffer is built with the reference's `ignore_load` rule (run.py:1376-1410): every key present on both
        sides is loaded, a shape mismatch on such a key is a ValueError, everything else keeps its own initialisation.
        `.init_missing`: the model keys the dict lacked; `.init_unused`: the dict keys the model lacks (the two lists the
        reference prints).
        bn_stages (a "-bn" workload; False: nothing changes): the batch-norm backbone runs as step-executor stages, one
        autograd node per level (unet.SparseUNet; the developer switch SCN_EXEC_BN=1 does the same for a step built without
        the keyword).  Same kernels, arguments and bits as the layer-by-layer path, which stays the default.
        bottleneck_divisor, main_path_relu (0 / False: nothing changes): the backbone's residual units take the reference's
        bottleneck form (inner width C // bottleneck_divisor) and / or its main-path ReLU (unet.residual_block).  dtype="bf16"
        needs every inner width to be a multiple of 8 (ValueError otherwise).  The mask branch keeps the plain unit.
        relu_first, drop_input_relu, use_residuals (True: nothing changes): the backbone's post-activation units
        (relu_first=False), the ReLU of its encoder input stages kept (drop_input_relu=False), plain convolution blocks in place
        of residual units (use_residuals=False; with a non-default bottleneck_divisor / main_path_relu: ValueError).
        loss_weights (None: nothing changes): a dict over `rpn_class`, `rpn_bbox`, `class`, `mask`, `segmentation` with the
        reference's `loss_*_weight` values (default 1 each; run.py keeps `loss_segmentation_weight=1/8` as an option).  A key of
        a loss that is off, an unknown key or a value that is not positive and finite: ValueError.
        multitask_loss (False: nothing changes): the five log-weights -log(weight) are parameters of the step's model
        (`model.loss_combiner`, loss.LossCombiner: the reference's `Loss(multitask_loss=True)`, loss.py:44-58), sit in the flat
        buffer, are all-reduced with the rest and updated by FlatAdam / SGD.
        With multitask_loss, or any weight other than 1, the step owns the reference's loss container: per micro-batch ONE
        scn_loss_combine launch between forward and backward writes the gradients the loss roots are back-propagated with --
        exp(-log-weight) / batches_per_step each, the two RPN roots with the reference's crossed weights (loss.py:111-114) -- and
        adds the log-weights' gradients into their views of the flat gradient buffer.  `.loss_record`: the reference's
        `sublosses` mapping of the last micro-batch (loss.LossRecord, on the device until read); `.loss_weights()`: the
        reference's `get_weights()`.  Otherwise no container is built and no such launch is made.
        simple_class (with dense_class=True; False: nothing changes): the class branch is the reference's class network WITHOUT
        pooling (classhead.ReshapeClassBranch; `simple_class`, run.py:706-710, the `cs8_dense8max4_reshape` runs): RoiAlign to 8^3
        straight out of the RPN stack's volume at its full width, max pool 2, one 3^3 same-convolution to 8 channels, flatten,
        ReLU Linear(512, 64) ReLU Linear(64, 18) -- RoiAlign and max pool as one pass (scn_roialign_pool_fwd / _bwd).  fp32: in a
        bf16 step the head widens the volume on entry; with class_storage="bf16" ValueError.  Selector, losses, predict() and
        evaluate() are those of the dense arm.
        class_storage (with dense_class=True and dtype="bf16"; None: nothing changes): "bf16" keeps the dense class branch's
        slabs bf16-stored (classhead.DenseClassBranch(storage=torch.bfloat16): input convolution, RoiAlign, max pool and strided
        levels on bf16 slabs with fp32 accumulation; linear layers and scores fp32) and hands it the RPN stack's volume as the
        stack stored it, instead of widening the volume to an fp32 branch.
        upsample_heads (`ref-crop-rpn` only; False: nothing changes): the RPN heads are the reference's committed ones
        (run.py:339 `upconvoluted_anchornetwork = True`): rpn.AnchorNetworkUpsample, per anchor level one transposed
        convolution per group of anchors that share an extra stride, so targets, draw, top-k and NMS see the reference's anchor
        set (182 272 anchors per 128 x 128 x 64 crop, 88 536 inside) instead of the 1x1 heads' 71 680; every loss, predict() and
        evaluate() run on it without further switches.  Any dtype: where the RPN's level tensors are bf16-stored (dtype "bf16")
        the dilation stacks stay bf16-stored through their last ReLU (scn_relu_fwd_bf16); the heads' row GEMM, P, the scatter
        and rpn_bbox / rpn_score are fp32, as behind the 1x1 heads.
        step_group: run the fp32 weight gradients of a step as one grid per kernel variant after the last backward pass
        (executor.step_weight_gradients; one rank, no gradient buckets).  It keeps every stage's workspaces and unit slabs alive
        until then -- the cfg2 step's working set grows from 1.04 to 2.03 GB -- so False is the way to fit a scene that only fits
        with the per-pass form.
        batches (the `-rpn` workloads only; default None = the synthetic scenes): `batches_per_step` collated batches
        (`sample.collate` of `sample.convert_sample` outputs: the reference's batch dict) that take the place of the synthetic
        scenes -- coordinates, features, spatial size, splits, ground-truth boxes, labels, packed instance masks and per-point
        segmentation labels all come from the batch, so every loss, predict() and evaluate() run on converted data.  The
        spatial size must be a multiple of 2^(levels - 1) of the workload's network, times 4 with class_loss on the sparse arm (convert with
        `required_size_factor`: 8, or 32, for the 4-level cfg3-rpn), else ValueError; instance labels must lie in 0 .. 17 and segmentation labels in 0 .. 19 or be -100.
        rpn_loss (the `-rpn` workloads only): train the RPN on the reference's RPN loss (loss.RpnLoss with
        BatchwiseBboxTargetSelector(0.35, 0.15, 1/8), sigma 2; scannet_config/run.py:359-368,876-884) against the scene's
        synthetic boxes, in place of the fixed synthetic gradient on rpn_bbox / rpn_score.  Targets and draw are queued before
        the backbone forward; the two loss values stay on the device as `.rpn_losses`.
        mask_loss (the `-rpn` workloads only): train the mask branch on the reference's mask loss (scannet_config/run.py:
        398,799-810,857-862,876-891): after the proposal selection, loss.TrainSelector(0.2, 0, (24, 0, True)) draws up to 24
        proposals per sample with IoU >= 0.2 against the scene's synthetic ground truth and appends every ground-truth box (one
        launch), the mask branch crops and runs on those boxes, and loss.MaskLoss (BCE-with-logits of the instance's label
        column against its mask, synthetic.make_instances) is backpropagated with gradient 1 / batches_per_step.  This
        replaces both the seeded synthetic gradient on the mask logits and ref-crop-rpn's cut to the 24 best-scored
        proposals.  The loss stays on the device as `.mask_losses`.  Without it the mask branch gets the synthetic gradient.
        class_loss (the `-rpn` workloads only): add the reference's class branch (classhead.ClassBranch on the coarsest RPN
        level of the encoder) and train it on the reference's class loss (run.py:399,520-521,729-732): after the proposal
        selection, loss.TrainSelector(0.1, 0, (32, 0, True)) draws up to 32 proposals per sample with IoU >= 0.1 -- from the
        overlap descriptions the mask selector computed when both are on (model.py:170-183) -- and appends every ground-truth
        box; the branch runs on those boxes, loss.ClassLossSelector + loss.ClassLoss give `.class_losses` (on the device),
        back-propagated with 1 / batches_per_step.
        dense_class (with class_loss): the class branch is the reference's DENSE one (classhead.DenseClassBranch, run.py:340
        `dense_class = True`): RoiAlign to 16^3 out of the volume the RPN's dilation stack produced, so the class loss trains
        that stack too; everything around it (selector, ClassLossSelector, ClassLoss, predict(), evaluate()) is the same.  A
        batch's spatial size then needs no factor beyond the backbone's.  False: the sparse arm, unchanged.
        segmentation_loss (the workloads with boxes: cfg3, cfg3-rpn, ref-crop-rpn): add the reference's segmentation head
        (classhead.SegmentationHead, 20 classes) on the backbone output and train it on loss.CrossEntropyLoss against
        synthetic.make_segmentation of the scene's instances.  Its gradient REPLACES the seeded N(0, 1) gradient on the
        backbone output; the loss stays on the device as `.segmentation_losses`.
        With several losses on, the roots are summed with weight 1: the reference's `Loss` as configured (multitask_loss=False,
        every weight 1, loss.py:44-58, run.py:876-898) -- unless loss_weights / multitask_loss say otherwise (above).
        n_gt (the `-rpn` workloads): the ground-truth instances per sample both losses see are the first n_gt synthetic boxes
        (None: all of them; ref-crop-rpn has 256 per crop, which would put > 3000 boxes through the mask branch).
        optimizer: "sgd" (plain SGD on the flat buffer) or "adam" (the reference's optimizer, scannet_config/run.py:403-416,
        1449: the fused Adam launch of optim.FlatAdam with `betas`, `eps`, `weight_decay`; lr=None -> the reference's 4e-4).
        On a CPU device either optimizer's step constructs (to be inspected and described) and refuses when it is stepped.
        batches_per_step: micro-batches whose gradients are accumulated before ONE all-reduce + update, each scaled by
        1 / batches_per_step -- the reference's `(loss / batches_per_step).backward()` ... `optimizer.step()`
        (ndsis/training/training.py:436,458-460; 2 or 6 with the mask head, scannet_config/run.py:377-396).  Micro-batch k
        is its own scene (seed + 1000 k); all but the last run under `FlatParams.accumulate()`.
        weighting: how the ranks' gradients are averaged -- "equal" (1 / world: balanced scenes, the benchmark) or "count"
        (each rank in proportion to its active voxels: what a loss normalised by batch-level counts gives when the
        batch is sharded one scene per rank, loss.py:401-431; the counts are summed over ranks once per step)."""
        ch, gr, tg, nb, self.baseline_entry, n_samples = WORKLOADS[workload]
        self.with_rpn = workload.endswith("-rpn")
        requested = {"rpn": bool(rpn_loss), "class": bool(class_loss), "mask": bool(mask_loss), "segmentation": bool(segmentation_loss)}
        # 1. option checks, before anything is allocated
        self._check_heads(workload, requested, nb, dtype, dense_class, class_storage, simple_class, upsample_heads, n_gt)
        self._check_loss_weights(requested, loss_weights, multitask_loss)
        batches = self._check_run(workload, dtype, prefetch, batches, n_gt, batches_per_step, optimizer, lr, weighting, step_group)
        self.channels, self.grid = tuple(channels or ch), tuple(grid or gr)
        self.n_boxes = nb if n_boxes is None else n_boxes
        if dtype not in ("f32", "bf16", "bf16-blocks"):
            raise ValueError("dtype: f32 | bf16 | bf16-blocks")
        self._check_train(train, requested, multitask_loss)
        self._max_grad_norm = None               # (read through the `max_grad_norm` property)
        if max_grad_norm is not None:
            bound = float(max_grad_norm)
            if not (bound > 0 and bound < float("inf")):
                raise ValueError(f"max_grad_norm: a positive finite bound required (None: no clipping), got {max_grad_norm!r}")
            self._max_grad_norm = bound
        if requested["segmentation"] and not self.n_boxes:
            raise ValueError("segmentation_loss=True needs boxes (n_boxes > 0)")
        # 2. the scenes, resident on the device
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._build_scenes(batches, n_samples, target or tg, seed)
        # 3. the model.  The order of construction under one seed decides every initial value: class branch and segmentation
        # head last (SparseStepModel), the loss container after the model, the RPN heads' own initialisation after that
        torch.manual_seed(0)
        self._build_model(dtype, bottleneck_divisor, main_path_relu, relu_first, drop_input_relu, use_residuals, bn_stages)
        # 4. the loss objects, 5. the ground-truth instances they are computed against
        self._build_losses(seed)
        if self.mask_loss or self.class_loss or self.segmentation_loss:
            self._build_instances(seed)
        # 6. an earlier stage's values, 7. what is frozen, 8. the flat buffer over the rest, 9. the container's views of it
        self.init_missing = self.init_unused = None
        if init_state is not None:
            self.init_missing, self.init_unused = self._load_init_state(init_state)
        self._build_flat(n_buckets)
        if self.combiner is not None:
            self._build_container_views()
        # 10. the optimizer
        self.adam = None
        if optimizer == "adam":
            from .optim import FlatAdam
            self.adam = FlatAdam(self.flat, lr=self.lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._gen = torch.Generator(device="cpu").manual_seed(grad_seed)
        self._gys, self._gms, self._grs = {}, {}, {}
        self._gm_pool = self._md_next = None
        self.n_active = self.n_roi_rows = 0
        self.out = self.logits = self.fin = self.rpn_out = None

    # ---- the constructor's phases, in the order they run ---------------------------------------------------------------
    def _check_heads(self, workload, requested, nb, dtype, dense_class, class_storage, simple_class, upsample_heads, n_gt):
        for name in ("rpn", "mask", "class"):
            if requested[name] and not self.with_rpn:
                raise ValueError(f"{name}_loss=True needs an RPN in the step (the -rpn workloads)")
        if dense_class and not requested["class"]:
            raise ValueError("dense_class=True chooses the class branch's arm: it needs class_loss=True")
        if class_storage not in (None, "bf16"):
            raise ValueError("class_storage: None | 'bf16'")
        if class_storage and not (dense_class and dtype == "bf16"):
            raise ValueError("class_storage='bf16' needs dense_class=True and dtype='bf16'")
        self.class_storage = class_storage
        if simple_class and not dense_class:
            raise ValueError("simple_class=True is a head of the dense arm: it needs dense_class=True")
        if simple_class and class_storage:
            raise ValueError("simple_class=True computes in fp32: class_storage='bf16' belongs to the pooling dense head")
        self.simple_class = bool(simple_class)
        if upsample_heads and workload != "ref-crop-rpn":
            raise ValueError("upsample_heads=True is the reference's RPN head: only ref-crop-rpn has its two anchor levels")
        self.upsample_heads = bool(upsample_heads)
        if requested["segmentation"] and not nb:
            raise ValueError("segmentation_loss=True needs a workload with boxes (cfg3, cfg3-rpn, ref-crop-rpn): the labels "
                             "come from the scene's instances")
        if n_gt is not None and not self.with_rpn:
            raise ValueError("n_gt applies to the ground truth of the -rpn workloads")
        if n_gt is not None and int(n_gt) < 1:
            raise ValueError("n_gt >= 1 required")
        self.n_gt = None if n_gt is None else int(n_gt)
        self.dense_class = bool(dense_class)
        self.rpn_loss, self.class_loss, self.mask_loss, self.segmentation_loss = requested.values()

    def _check_loss_weights(self, requested, loss_weights, multitask_loss):
        loss_on = {"rpn_class": requested["rpn"], "rpn_bbox": requested["rpn"], "class": requested["class"],
                   "mask": requested["mask"], "segmentation": requested["segmentation"]}
        weights = dict.fromkeys(loss_on, 1.0)
        if loss_weights is not None:
            if not isinstance(loss_weights, dict):
                raise ValueError("loss_weights: a dict over " + ", ".join(loss_on) + " required")
            for key, v in loss_weights.items():
                if key not in loss_on:
                    raise ValueError(f"loss_weights: unknown key {key!r} (the keys: " + ", ".join(loss_on) + ")")
                if not loss_on[key]:
                    raise ValueError(f"loss_weights[{key!r}]: that loss is off in this step")
                v = float(v)
                if not (v > 0 and v < float("inf")):
                    raise ValueError(f"loss_weights[{key!r}]: a positive finite weight required, got {v}")
                weights[key] = v
        if multitask_loss and not any(loss_on.values()):
            raise ValueError("multitask_loss=True needs at least one of rpn_loss, mask_loss, class_loss, segmentation_loss: it "
                             "learns the weights of those losses")
        # the loss container exists only when it has something to do: a learned or a non-unit weight
        self._loss_weights = weights if (multitask_loss or any(v != 1.0 for v in weights.values())) else None
        self.multitask_loss = bool(multitask_loss)

    def _check_run(self, workload, dtype, prefetch, batches, n_gt, batches_per_step, optimizer, lr, weighting, step_group):
        if batches is not None:
            if not self.with_rpn:
                raise ValueError("batches= applies to the -rpn workloads (the ground truth feeds the RPN, mask and class losses)")
            if n_gt is not None:
                raise ValueError("n_gt cuts the synthetic ground truth; a batch brings its own")
            batches = list(batches)
            if len(batches) != int(batches_per_step):
                raise ValueError(f"batches: {int(batches_per_step)} collated batches required (batches_per_step), got {len(batches)}")
        self.workload, self.dtype, self.prefetch = workload, dtype, prefetch
        # lr=None: the workload's default (reported by describe() and in bench.py's line).  1e-6, and 1e-8 with an RPN in the
        # step: the SAME synthetic gradient on 3.7 M RPN outputs every step is a steady push, not noise -- at 1e-6 the score
        # field grows 4 % per step and overflows within a bench run (profiles/r5_rpn_stats.txt); the update itself (one SGD
        # pass over the flat buffer) is the same work.  An explicit lr is used as given.
        if optimizer not in ("sgd", "adam"):
            raise ValueError("optimizer: sgd | adam")
        self.optimizer = optimizer
        default_lr = 4e-4 if optimizer == "adam" else (1e-8 if self.with_rpn else 1e-6)
        self.lr = default_lr if lr is None else float(lr)
        if weighting not in ("equal", "count"):
            raise ValueError("weighting: equal | count")
        self.weighting = weighting
        self.step_group = bool(step_group)
        self.batches_per_step = int(batches_per_step)
        if self.batches_per_step < 1:
            raise ValueError("batches_per_step >= 1")
        if self.batches_per_step > 1 and weighting == "count":
            raise ValueError("count-weighted ranks with gradient accumulation: scale each micro-batch's loss by its own count "
                             "instead (rank_weight applies to the accumulated sum when a slice is packed)")
        self._total_weight = None
        return batches

    def _check_train(self, train, requested, multitask_loss):
        have = {"backbone": True, "rpn": self.with_rpn, "class": self.class_loss, "mask": bool(self.n_boxes),
                "segmentation": self.segmentation_loss}
        if train is not None:
            if isinstance(train, str):
                raise ValueError("train: a tuple of part names required, e.g. train=('mask',), got the string " + repr(train))
            train = tuple(train)
            if not train:
                raise ValueError("train: an empty tuple trains nothing; None trains every part")
            for name in train:
                if name not in PARTS:
                    raise ValueError(f"train: unknown part {name!r} (the parts: " + ", ".join(PARTS) + ")")
                if not have[name]:
                    raise ValueError(f"train: this step has no part {name!r} (it has: " + ", ".join(p for p in PARTS if have[p]) + ")")
            if multitask_loss:
                raise ValueError("multitask_loss=True together with train: the learned log-weights of a step that trains only "
                                 "some parts are not provided")
        self.train = train
        self.trainable = tuple(p for p in PARTS if have[p] and (train is None or p in train))
        self.frozen = tuple(p for p in PARTS if have[p] and p not in self.trainable)
        on = set(self.trainable)
        # a requested loss is computed only if its gradient reaches a trainable parameter (run.py:891-893 `calc_* and not mask_only`)
        under = {"rpn": {"rpn", "backbone"}, "class": {"class", "backbone", "rpn"} if self.dense_class else {"class", "backbone"},
                 "mask": {"mask", "backbone"}, "segmentation": {"segmentation", "backbone"}}
        self._computed = {k: requested[k] and bool(on & under[k]) for k in requested}
        self.losses_not_computed = tuple(k for k in requested if requested[k] and not self._computed[k])
        # the mask branch runs in forward_backward when something trainable lies under its logits
        self._run_mask = bool(self.n_boxes) and bool(on & {"mask", "backbone"})

    def _build_scenes(self, batches, n_samples, target, seed):
        self._scenes = []
        self.from_batches = batches is not None
        # level constraint on a batch's spatial size: every 2^3/2 convolution halves an even size -- levels - 1 in the backbone,
        # two more in the SPARSE class branch, which cuts its boxes out of the coarsest level's grid (the dense one resamples
        # every box to its own 16^3 grid: the volume's stride is one of the backbone's)
        self._size_factor = 2 ** (len(self.channels) - 1) * (4 if self.class_loss and not self.dense_class else 1)
        for k in range(self.batches_per_step):
            if self.from_batches:
                self._scenes.append(self._scene_from_batch(batches[k], k))
                continue
            coords, feats, size, bs, splits = make_batch(n_samples, self.grid, target, dup=1.15, seed=seed + 1000 * k)
            boxes = make_boxes(coords, self.n_boxes, seed=seed + 1000 * k + 2) if self.n_boxes else None
            gt_boxes = boxes if (boxes is None or self.n_gt is None) else [b[:self.n_gt] for b in boxes]
            self._scenes.append(dict(coords_cpu=coords, feats_cpu=feats, size=size, batch_size=bs, splits=splits,
                                     coords=coords.to(self.device), feats=feats.to(self.device), boxes=boxes,
                                     gt_boxes=gt_boxes))   # resident in HBM
        self._use_scene(0)

    def _build_model(self, dtype, bottleneck_divisor, main_path_relu, relu_first, drop_input_relu, use_residuals, bn_stages):
        # ref-crop-rpn: 256 proposals per sample survive the selection (run.py:847-853); the mask network then works on the
        # <= 24 its TrainSelector draws from them (mask_network_params.selection_tuple = (24, 0, True), run.py:799-810;
        # model.py:919-1014 draws by ground-truth overlap -- out of scope: here the 24 best-scored ones)
        self.mask_boxes = 24 if self.workload == "ref-crop-rpn" else None
        rpn_kind = "reference" if self.workload == "ref-crop-rpn" else ("stand-in" if self.with_rpn else False)
        self.bottleneck_divisor, self.main_path_relu = int(bottleneck_divisor or 0), bool(main_path_relu)
        self.relu_first, self.drop_input_relu, self.use_residuals = bool(relu_first), bool(drop_input_relu), bool(use_residuals)
        self.bn_stages = bool(bn_stages)
        storage = {"f32": False, "bf16": "all", "bf16-blocks": True}[dtype]
        self.model = SparseStepModel(self.channels, bool(self.n_boxes), storage, rpn_kind, self.n_boxes,
                                     batchnorm=self.workload.endswith("-bn"),
                                     with_class="dense" if self.dense_class else self.class_loss,
                                     with_segmentation=self.segmentation_loss, upsample_heads=self.upsample_heads,
                                     class_storage=self.class_storage, simple_class=self.simple_class,
                                     bottleneck_divisor=self.bottleneck_divisor, main_path_relu=self.main_path_relu,
                                     relu_first=self.relu_first, drop_input_relu=self.drop_input_relu,
                                     use_residuals=self.use_residuals, bn_stages=self.bn_stages).to(self.device)
        self.combiner = self.loss_record = None
        if self._loss_weights is not None:
            from .loss import LossCombiner
            do = self._computed
            self.combiner = self.model.loss_combiner = LossCombiner(
                tuple(self._loss_weights.values()), self.multitask_loss,
                has=(do["rpn"], do["class"], do["mask"], do["segmentation"])).to(self.device)
        if self.with_rpn:
            self._init_rpn()

    def _build_losses(self, seed):
        from . import loss as RL
        # the gradient every loss root is back-propagated with when no container weighs it: 1 / batches_per_step on the device
        self._loss_grad = torch.full((), 1.0 / self.batches_per_step, dtype=torch.float32, device=self.device)
        self.rpn_losses = self.mask_losses = self.class_losses = self.segmentation_losses = None
        self.mask_out = self.class_out = self.segmentation_out = None
        # (tests: retain the gradients that reach rpn_bbox / rpn_score, the mask logits, the class scores / segmentation logits)
        self.keep_rpn_grads = self.keep_mask_grads = self.keep_class_grads = False
        if self.rpn_loss:
            self.rpn_criterion = RL.RpnLoss(RL.BatchwiseBboxTargetSelector(0.35, 0.15, max_weight=1 / 8, seed=seed), sigma=2.)
            self._rpn_targets = {}
        if self.mask_loss:
            # run.py:799-810: mask_network_params.selection_tuple = (24, 0, True) behind TrainSelector(0.2); MaskLoss without
            # class weights (run.py:398, 876-891)
            self.mask_selector = RL.TrainSelector(0.2, 0, (24, 0, True), seed=seed + 17)
            self.mask_criterion = RL.MaskLoss(class_weights=None)
        if self.class_loss:
            # run.py:399,520-521,729-732: positive_threshold 0.1, selection_tuple (32, 0, True); ClassLoss without weights
            self.class_selector = RL.TrainSelector(0.1, 0, (32, 0, True), seed=seed + 29)
            self.class_loss_selector = RL.ClassLossSelector(0.1)
            self.class_criterion = RL.ClassLoss(class_weights=None)
        if self.segmentation_loss:
            self.segmentation_criterion = RL.CrossEntropyLoss(weight=None, ignore_index=-100)

    def _build_instances(self, seed):
        """Instances built (and packed, for the mask loss) once per scene; a converted batch brought its own
        (_scene_from_batch)."""
        from .loss import pack_gt_masks
        for k, sc in enumerate(self._scenes):
            if self.from_batches:
                continue
            labels, masks = make_instances(sc["coords_cpu"], sc["gt_boxes"], n_classes=self.model.mask.classes,
                                           seed=seed + 1000 * k + 5)
            sc["gt_label"] = list(torch.cat(labels).to(self.device).split([l.shape[0] for l in labels]))    # views of one tensor
            sc["gt_mask_cpu"] = masks
            if self.mask_loss:
                sc["gt_mask"] = pack_gt_masks([mk.to(self.device) for mk in masks])
            sc["gt_dev"] = [b.float().to(self.device) for b in sc["gt_boxes"]]
            if self.segmentation_loss:             # one label per point row, in the batch's row order (sample-major)
                sc["seg_target"] = torch.cat(make_segmentation(labels, masks)).to(self.device)

    def _build_flat(self, n_buckets):
        """Freeze the parts `train=` does not name, then the flat buffer over what is left; equal on every rank."""
        frozen_params = []
        if self.train is not None:
            for name in self.frozen:
                for p in self._part(name).parameters():
                    p.requires_grad_(False)
                    frozen_params.append(p)
        if self.max_grad_norm is not None and not any(p.requires_grad for p in self.model.parameters()):
            raise ValueError("max_grad_norm: the parts this step trains (" + ", ".join(self.trainable) + ") have no parameters, "
                             "there is no gradient to clip")
        self.flat = FlatParams(self.model, n_buckets=n_buckets)
        self.flat.max_grad_norm = self.max_grad_norm
        broadcast_params(self.flat)
        broadcast_tensors([p.data for p in frozen_params])      # (more than one rank: the frozen parameters are equal everywhere too)

    def _build_container_views(self):
        self._root_grad = torch.zeros(L.LOSS_TERMS, dtype=torch.float32, device=self.device)
        self._root_grad_views = [self._root_grad[i] for i in range(L.LOSS_TERMS)]
        self._weight_params = self._weight_grad_views = self._weight_grad_slab = None
        if self.multitask_loss:
            # the five log-weights are the model's last parameters: their gradient views lie back to back in the flat buffer
            index = {id(p): i for i, p in enumerate(self.flat.params)}
            self._weight_params = self.combiner.log_weights()
            self._weight_grad_views = [self.flat.grad_views[index[id(p)]] for p in self._weight_params]
            first = self._weight_grad_views[0].storage_offset()
            if [v.storage_offset() for v in self._weight_grad_views] != list(range(first, first + L.LOSS_TERMS)):
                raise L.ScnError("SceneStep: the log-weights are not adjacent in the flat gradient buffer")
            self._weight_grad_slab = self.flat.flat_grad[first:first + L.LOSS_TERMS]
            on = (self.rpn_loss, self.rpn_loss, self.class_loss, self.mask_loss, self.segmentation_loss)
            self._weights_on = [p for p, o in zip(self._weight_params, on) if o]
            self._weight_grad_views = [v if o else None for v, o in zip(self._weight_grad_views, on)]

    # ------------------------------------------------------------------------------------------------------------
    def _part(self, name):
        """The sub-module of the step's model that `train=` calls `name` (PARTS)."""
        m = self.model
        return {"backbone": m.backbone, "rpn": m.rpn, "class": m.class_branch, "mask": m.mask, "segmentation": m.segmentation}[name]

    def _load_init_state(self, state):
        """The reference's `ignore_load` (run.py:1376-1410) on the step's model: every key of `state` the model has is copied
        in (a shape mismatch: ValueError), everything else keeps its initialisation.
        -> (model keys `state` lacks, keys of `state` the model lacks)."""
        own = self.model.state_dict()
        for key, v in own.items():
            got = state.get(key)
            if got is not None and tuple(got.shape) != tuple(v.shape):
                raise ValueError(f"init_state[{key!r}]: shape {tuple(got.shape)} where the model has {tuple(v.shape)}")
        with torch.no_grad():
            for key, v in own.items():
                if key in state:
                    v.copy_(state[key].to(device=v.device, dtype=v.dtype))
        return [k for k in own if k not in state], [k for k in state if k not in own]

    def _scene_from_batch(self, batch, k):
        """The scene dict of micro-batch k from a collated batch (sample.collate / the reference's collate_fn layout)."""
        from .loss import PackedMasks, pack_gt_masks
        coords, feats, size, batch_size, splits = batch["data"]
        size = torch.as_tensor(size).to("cpu", torch.long)
        factor = self._size_factor
        if any(int(v) % factor or int(v) < factor for v in size):
            raise ValueError(f"batches[{k}]: spatial size {tuple(int(v) for v in size)} is not a multiple of {factor} on every axis, "
                             f"which the {len(self.channels)}-level network of '{self.workload}'"
                             + (" with the class branch's two further 2^3/2 convolutions" if factor > 2 ** (len(self.channels) - 1)
                                else "") + f" needs: convert the samples with required_size_factor={factor}")
        if feats.shape[1] != 7:
            raise ValueError(f"batches[{k}]: 7 feature columns (colour, ones, normal) required, got {feats.shape[1]}")
        gt = [b.to(self.device, torch.float32) for b in batch["gt_bbox"]]
        gt_mask = batch["gt_mask"]
        if not isinstance(gt_mask, PackedMasks):
            gt_mask = pack_gt_masks([mk.to(self.device) for mk in gt_mask])
        return dict(coords_cpu=None, feats_cpu=None, size=size, batch_size=int(batch_size), splits=list(splits),
                    coords=coords.to(self.device), feats=feats.to(self.device, torch.float32).contiguous(), boxes=gt, gt_boxes=gt,
                    gt_dev=gt, gt_label=[l.to(self.device) for l in batch["gt_label"]], gt_mask=gt_mask, gt_mask_cpu=None,
                    seg_target=batch["gt_segmentation"].to(self.device))

    def _use_scene(self, k):
        sc = self._scenes[k]
        for key in ("coords_cpu", "feats_cpu", "size", "batch_size", "splits", "coords", "feats", "boxes", "gt_boxes"):
            setattr(self, key, sc[key])
        self._k = k

    def _scene_shape(self):
        return tuple(float(v) for v in self.size)

    def _rpn_target_setup(self, k):
        """(calculator over the inside anchors of micro-batch k's scene, its boxes concatenated on the device, host offsets):
        a function of the scene shape and the scene's boxes only, built once."""
        got = self._rpn_targets.get(k)
        if got is None:
            rpn = self.model.rpn
            stride = 1 if hasattr(rpn, "levels") else rpn.stride      # (the levels take the scene's shape, one level its own grid's)
            calc = rpn.target_calculator(tuple(int(v) // stride for v in self.size), self.device)
            offs = [0]
            for b in self.gt_boxes:
                offs.append(offs[-1] + b.shape[0])
            gt = torch.cat([b.reshape(-1, 6) for b in self.gt_boxes], 0).float().to(self.device) if offs[-1] else None
            got = self._rpn_targets[k] = (calc, gt, offs)
        return got

    def _init_rpn(self):
        """Random-init heads give near-constant scores; the synthetic RPN gets a head whose scores spread (so that top-k and
        NMS have something to decide) -- seeded, the same on every rank."""
        g = torch.Generator().manual_seed(1234)
        rpn = self.model.rpn
        up = getattr(rpn, "anchor_network", None)                 # (the up-sampling heads' weights: [C, A_g * 7, s0, s1, s2])
        heads = up.heads() if up is not None else ([r.head for r in rpn.levels] if hasattr(rpn, "levels") else [rpn.head])
        with torch.no_grad():
            for h in heads:
                w = torch.randn(h.weight.shape, generator=g) * 0.02              # box deltas: boxes stay near their anchors
                scores = w[:, 6::7] if up is not None else w[6::7]               # channel a*7+6 = the score of anchor a
                scores.copy_(torch.randn(scores.shape, generator=g) * 0.5)
                h.weight.copy_(w.to(h.weight.device))
                h.bias.zero_()

    def _take_index(self, k):
        """The index structures of micro-batch k if a helper thread built them (else None: the forward builds them)."""
        md = self._md_next.result() if self._md_next is not None else None
        self._md_next = None
        return md

    def _start_prefetch(self, k):
        if self.prefetch and self._md_next is None:
            nx = self._scenes[(k + 1) % self.batches_per_step]
            self._md_next = self.model.backbone.prefetch_in_thread(nx["coords"], nx["size"], nx["batch_size"])

    def _combine_losses(self, ledger, zero):
        """The loss container's launch of one micro-batch, between forward and backward: the gradient of term i's root becomes the
        device scalar exp(-log-weight of term i) / batches_per_step, and with multitask_loss the log-weights' gradients are
        added into their views of the flat gradient buffer (zeroed at the step's first micro-batch), which become their
        `.grad`."""
        from . import loss as RL
        cb = self.combiner
        views = None
        if self.multitask_loss:
            # only the weights of the losses that are on get a gradient: the others keep `grad is None`, as in the reference
            views = self._weight_grad_views
            if zero:
                self._weight_grad_slab.zero_()
            self.flat.adopt_views(self._weights_on)
        record = RL.loss_combine(ledger.terms, cb.log_weights(), 1.0 / self.batches_per_step, root_grad=self._root_grad,
                                 weight_grads=views, running=cb._running_for(self._root_grad.device))
        self.loss_record = RL.LossRecord(record, [t is not None for t in ledger.terms])
        for i, pos in ledger.term_pos.items():
            ledger.grads[pos] = self._root_grad_views[i]
        if self.multitask_loss and self.flat.sync:
            self.flat.mark_ready(self._weights_on)       # (bucketed all-reduce: autograd never reaches these parameters)

    def loss_weights(self):
        """The reference's `Loss.get_weights()` for the losses of this step: exp(-log-weight) under its keys `rpn_score`,
        `rpn_bbox`, `class`, `mask`, `segment` (one copy; without a container every weight is 1)."""
        if self.combiner is not None:
            return self.combiner.get_weights()
        keys = (("rpn_score", "rpn"), ("rpn_bbox", "rpn"), ("class", "class"), ("mask", "mask"), ("segment", "segmentation"))
        return {key: 1.0 for key, loss in keys if self._computed[loss]}

    def upstream_grads(self, k=0):
        """(dY of the backbone output, dY of the mask logits or None) of micro-batch k, BEFORE the 1 / batches_per_step scale."""
        return self._gys.get(k), self._gms.get(k)

    def forward_backward(self, k=0, zero=True):
        """Index build + forward + backward of micro-batch k (no collective, no update); the upstream gradients are scaled
        by 1 / batches_per_step.  zero: drop the gradients first (the first micro-batch of a step).
        Keeps .out / .logits / .fin for checks."""
        m = self.model
        # (the gradients are dropped right before backward, not here: at the step boundary the GPU's queue is empty, and 156
        #  attribute stores are 40-50 us the first forward kernels would wait for)
        if k != self._k:
            self._use_scene(k)
        # (a frozen backbone takes the features as they are: nothing below it asks for a gradient, its stages run forward-only)
        fin = self.feats.detach().requires_grad_() if "backbone" in self.trainable else self.feats
        md = self._take_index(k)
        # the index structures of the NEXT batch depend on its coordinates only (a data loader's output): a helper thread
        # builds them on the high-priority index stream while this batch runs; every step contains one complete build
        if not LATE_PREFETCH:
            self._start_prefetch(k)
        # cfg3-rpn: the RPN reads the ENCODER outputs only (model.py:141-160), so its heads, top-k and NMS are queued between
        # encoder and decoder, and the one host wait of the selection falls while the decoder's kernels run
        rpn_state = []

        def rpn_after_encoder(interims):
            rpn_bbox, rpn_score, anchors = m.run_rpn(interims)
            rpn_state.append((rpn_bbox, rpn_score, anchors, m.roi_selector.start(rpn_bbox, rpn_score, anchors, self._scene_shape())))
        hook = rpn_after_encoder if (self.with_rpn and RPN_BEFORE_DECODER) else None
        # cfg3: the ROI crop's selection and the ROI batch's index structures depend on coordinates and boxes only -- the
        # boxes of a step are known before its backbone runs (here: synthetic; in the reference: the RPN's proposals of
        # the same forward, so this applies to the mask branch's SECOND use of a scene, e.g. evaluation on cached proposals)
        cut = None
        if m.mask is not None and EARLY_ROI_CUT and not self.mask_loss and self._run_mask:
            cut = m.mask.prepare_cut(self.coords, self.size, self.boxes)      # (resident int64 coords: no dependency on md)
        rpn_prep = self._queue_rpn_targets(k) if self._computed["rpn"] else None
        out = m.backbone(self.coords, fin, self.size, self.batch_size, metadata=md, after_encoder=hook)
        self._start_prefetch(k)      # (LATE_PREFETCH: the helper thread is started once this batch's forward kernels are queued)
        ledger = _RootLedger()
        self._backbone_roots(ledger, k, out)
        if self.weighting == "count":             # before backward: the bucketed path scales slices as it packs them
            self._count_weight(out)
        boxes, logits = self.boxes, None
        proposals = overlaps = descs = None
        if self.with_rpn and m.mask is not None:
            if not rpn_state:
                rpn_after_encoder(m.backbone.unet.interims)
            boxes, proposals, overlaps, descs = self._rpn_roots(ledger, k, rpn_state[0], rpn_prep)
        if self._computed["class"]:
            self._class_roots(ledger, k, proposals, overlaps)
        if self._run_mask:             # (else: mask branch and backbone frozen -- nothing trainable lies under the logits)
            # (the crop's selection stays referenced until backward has run, as it always did: released earlier, its blocks --
            #  the ROI batch's coordinates among them -- would be handed to the backward pass's allocations)
            scene = (self.coords, fin, self.size, self.batch_size, self.splits)
            logits, selection = self._mask_roots(ledger, k, scene, out, boxes, descs, cut)
        if zero:
            self.flat.zero_grad()
        if self.combiner is not None:
            self._combine_losses(ledger, zero)
        if ledger.roots:               # (none: an empty crop in a step that trains the mask branch alone)
            _backward(ledger.roots, ledger.grads, step_scope=self.step_group and not self.flat.buckets and self.flat.sync)
        self.out, self.logits, self.fin = out, logits, fin

    # ---- the parts of forward_backward, in the order they run: each adds its roots to the ledger ------------------------
    def _seeded(self, cache, k, shape, draw):
        """The synthetic gradient of micro-batch k in `cache`: drawn from `self._gen` by `draw()` at first use and kept (the same
        direction every step; a draw per step would be timed as part of it), drawn again when the shape it was drawn for has
        changed.  -> (what the cache holds, whether it was drawn now)"""
        got = cache.get(k)
        lead = got[0] if type(got) is tuple else got
        if lead is not None and lead.shape == shape:
            return got, False
        got = cache[k] = draw()
        return got, True

    def _scaled(self, g):
        """The upstream gradient of one micro-batch out of `batches_per_step`."""
        return g if self.batches_per_step == 1 else g * (1.0 / self.batches_per_step)

    def _queue_rpn_targets(self, k):
        """The RPN loss's targets and draw depend on the anchors (the scene shape) and the boxes only: queued ahead of the
        backbone, they overlap nothing the forward waits for."""
        calc, gt, offs = self._rpn_target_setup(k)
        ov, am, tg = calc.from_concatenated(gt, offs)
        return (ov, am, tg) + tuple(self.rpn_criterion.bbox_target_selector(ov))

    def _backbone_roots(self, ledger, k, out):
        if self._computed["segmentation"]:
            # the reference's real gradient at the backbone output: the segmentation head's logits (fp32; bf16 storage widened)
            # against the scene's per-point labels, in place of the seeded N(0, 1) direction
            seg_logits = self.model.segmentation(out)
            if seg_logits.dtype != torch.float32:
                seg_logits = seg_logits.float()
            if self.keep_class_grads:
                seg_logits.retain_grad()
            seg_target = self._scenes[k]["seg_target"]
            self.segmentation_losses = self.segmentation_criterion(seg_logits, seg_target)
            self.segmentation_out = (seg_logits, seg_target)
            ledger.add(self.segmentation_losses, self._loss_grad, TERM_SEGMENTATION)
        elif out.features.requires_grad:
            shape = out.features.shape
            gy, drawn = self._seeded(self._gys, k, shape, lambda: torch.randn(shape, generator=self._gen).to(self.device))  # dY ~ N(0,1)
            if drawn:
                self.n_active = sum(g.shape[0] for g in self._gys.values())
            ledger.add(out.features, self._scaled(gy))
            return
        # (reached with the segmentation loss, or with nothing trainable under the backbone output: then there is no root here,
        #  and no synthetic gradient is drawn for one)
        self.n_active = int(out.features.shape[0]) * self.batches_per_step

    def _count_weight(self, out):
        import torch.distributed as dist
        self.flat.rank_weight = float(out.features.shape[0])
        tot = torch.tensor([self.flat.rank_weight], dtype=torch.float64)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            tot = tot.to(self.device if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(tot)
        self._total_weight = float(tot.item())

    def _rpn_roots(self, ledger, k, rpn_out, rpn_prep):
        """configs[2] as written (model.py:141-160): the proposals are this forward's -- dense heads on the coarsest encoder
        level, top-k + NMS on the device; the RPN losses' gradients arrive at rpn_bbox / rpn_score.
        -> (the boxes the mask branch runs on, the proposals, and -- with the mask loss -- its overlaps and descriptions)"""
        rpn_bbox, rpn_score, anchors, sel_state = rpn_out
        roi_score, boxes, roi_index = self.model.roi_selector.finish(sel_state)
        self.rpn_out = (rpn_bbox, rpn_score, anchors, roi_score, boxes, roi_index)
        descs = overlaps = None
        proposals = boxes
        if self._computed["mask"]:
            # model.py:172-196: OverlapCalculator + TrainSelector on this forward's proposals, one launch; the mask
            # branch runs on the drawn proposals ++ every ground-truth box
            overlaps, boxes, descs = self.mask_selector.select(boxes, self._scenes[k]["gt_dev"])
            boxes = list(boxes)
        elif self.mask_boxes is not None:     # (the reference's mask head trains on <= 24 selected proposals per sample)
            boxes = [b[:self.mask_boxes] for b in boxes]
        if self.keep_rpn_grads and rpn_bbox.requires_grad:
            rpn_bbox.retain_grad()
            rpn_score.retain_grad()
        if self._computed["rpn"]:
            calc = self._rpn_targets[k][0]
            if calc.anchors.data_ptr() != anchors.data_ptr() or calc.anchors.shape != anchors.shape:
                raise L.ScnError("SceneStep: the RPN loss's anchors are not the ones the RPN returned")
            self.rpn_losses = self.rpn_criterion.loss(rpn_prep, rpn_score, rpn_bbox)
            for term, value in zip((TERM_RPN_SCORE, TERM_RPN_BBOX), self.rpn_losses):       # (score_loss + bbox_loss) / batches_per_step
                ledger.add(value, self._loss_grad, term)
        elif rpn_bbox.requires_grad:               # (no RPN loss: the seeded direction, where a gradient can arrive)
            gr, _ = self._seeded(self._grs, k, rpn_bbox.shape, lambda: tuple(
                (torch.randn(t.shape, generator=self._gen) * 1e-3).to(self.device) for t in (rpn_bbox, rpn_score)))
            ledger.add(rpn_bbox, self._scaled(gr[0]))
            ledger.add(rpn_score, self._scaled(gr[1]))
        return boxes, proposals, overlaps, descs

    def _class_roots(self, ledger, k, proposals, overlaps):
        # model.py:170-183: the class network's TrainSelector draws from the same overlap descriptions as the mask
        # network's; the branch runs on its forward boxes (drawn proposals ++ every ground-truth box)
        m, sc = self.model, self._scenes[k]
        if overlaps is None:
            overlaps, cboxes, cdescs = self.class_selector.select(proposals, sc["gt_dev"])
        else:
            cboxes, cdescs = self.class_selector(overlaps)
        class_scores, csel = m.run_class(m.backbone.unet.interims, list(cboxes))
        if self.keep_class_grads:
            class_scores.retain_grad()
        sel_scores, sel_labels = self.class_loss_selector(class_scores, csel, cdescs, overlaps, sc["gt_label"])
        self.class_losses = self.class_criterion(sel_scores, sel_labels)
        self.class_out = (class_scores, csel, cdescs, sel_labels)
        ledger.add(self.class_losses, self._loss_grad, TERM_CLASS)

    def _mask_roots(self, ledger, k, scene, out, boxes, descs, cut):
        """-> the mask logits (an empty crop -- no proposal caught a point: the mask branch contributes nothing on this rank)
        and the crop's selection."""
        logits, selection = self.model.mask(scene, out, boxes, prepared_cut=cut)
        if self._computed["mask"]:
            sc = self._scenes[k]
            if self.keep_mask_grads and logits.requires_grad:
                logits.retain_grad()
            self.mask_out = (selection, descs)
            self.mask_losses = self.mask_criterion(logits, selection, descs, sc["gt_label"], sc["gt_mask"])
            ledger.add(self.mask_losses, self._loss_grad if self.mask_losses.requires_grad else None, TERM_MASK)
            self.n_roi_rows = int(logits.shape[0])
        else:
            gm, drawn = self._seeded(self._gms, k, logits.shape, lambda: self._draw_mask_grad(logits))
            if drawn:
                self.n_roi_rows = sum(g.shape[0] for g in self._gms.values())
            if logits.requires_grad and logits.shape[0]:
                ledger.add(logits, self._scaled(gm))
        return logits, selection

    def _draw_mask_grad(self, logits):
        if not self.with_rpn:
            return torch.randn(logits.shape, generator=self._gen).to(self.device)
        # the proposals -- and with them the number of cropped points -- change from step to step: dM is a slice
        # of one device-resident pool (drawing 2 M normals on the host per step would be timed as part of it)
        pool = self._gm_pool
        if pool is None or pool.shape[0] < logits.shape[0] or pool.shape[1:] != logits.shape[1:]:
            rows = max(2 * logits.shape[0], 1 << 18)
            pool = self._gm_pool = torch.randn((rows,) + tuple(logits.shape[1:]), generator=self._gen).to(self.device)
        return pool[:logits.shape[0]]

    def forward_only(self, k=0):
        """Evaluation forward of micro-batch k under torch.no_grad() -- what the reference's `eval_model`
        (ndsis/training/training.py:244-304) and `SparseMaskPredictor` (model.py:826-882) run: index build + backbone
        (+ ROI crop + mask branch), no graph, the executor's forward-only slab plan (executor._lean_layout), no
        backward-data weight images.  Same bits as the training forward.  -> (backbone output tensor, mask logits | None)"""
        run = self._infer(k, mask_boxes=self.mask_boxes)
        return run["out"], run.get("logits")

    # ---- the inference chain forward_only, predict and evaluate share --------------------------------------------------
    def _infer(self, k, with_class=False, mask_boxes=None, classify_too=None, own_index=False):
        """Micro-batch k under torch.no_grad(), on the index structures a helper thread built for it, the next build started
        (own_index: a pending build is joined and dropped -- it is for "the scene after the last one run", not for k -- and the
        forward builds its own): backbone -> RPN + proposal selection where the step has an RPN -> with_class: class branch + ClassPredictor on every
        kept box -> mask branch on the kept boxes (mask_boxes: on the first so many per sample), on the scene's own boxes in a
        step without RPN.  classify_too: further boxes for the class branch, run before the mask branch as evaluate() always ran
        them (the ground truth).  -> dict: `out`, `interims`; `roi_score`, `boxes`; `class`, `class_too` (_infer_class);
        `logits`, `selection`."""
        m = self.model
        if k != self._k:
            self._use_scene(k)
        md = None
        if own_index:
            self.finish()
        else:
            md = self._take_index(k)
            self._start_prefetch(k)
        with torch.no_grad():
            out = m.backbone(self.coords, self.feats, self.size, self.batch_size, metadata=md)
            run = dict(out=out, interims=m.backbone.unet.interims)
            if m.mask is None:
                return run
            boxes = self.boxes
            if self.with_rpn:
                rpn_bbox, rpn_score, anchors = m.run_rpn(run["interims"])
                roi_score, boxes, _ = m.roi_selector(rpn_bbox, rpn_score, anchors, self._scene_shape())
                run["roi_score"], run["boxes"] = list(roi_score), list(boxes)
                boxes = run["boxes"]
            if with_class:
                run["class"] = self._infer_class(run["interims"], boxes)
                if classify_too is not None:
                    run["class_too"] = self._infer_class(run["interims"], classify_too)
            if mask_boxes is not None and self.with_rpn:
                boxes = [b[:mask_boxes] for b in boxes]
            run["logits"], run["selection"] = self._infer_mask(out, boxes)
        return run

    def _infer_class(self, interims, boxes):
        """-> (class scores, the branch's selection, ClassPredictor's (indices, probabilities, raw indices)) on `boxes`."""
        from .loss import ClassPredictor
        class_scores, csel = self.model.run_class(interims, boxes)
        return class_scores, csel, ClassPredictor()(class_scores, csel)

    def _infer_mask(self, out, boxes):
        """-> (mask logits, (selection, counts, splits)) of the scene in use on `boxes`."""
        return self.model.mask((self.coords, self.feats, self.size, self.batch_size, self.splits), out, boxes)

    def _infer_segmentation(self, out):
        """-> (fp32 segmentation logits, SegmentationPredictor's (classes, probabilities))."""
        from .loss import SegmentationPredictor
        seg_logits = self.model.segmentation(out).float()
        return seg_logits, SegmentationPredictor(True)(seg_logits)

    def predict(self, k=0):
        """The reference's evaluation chain (model.py:185-219) on micro-batch k under torch.no_grad(): backbone -> RPN ->
        proposal selection -> class branch on all kept boxes -> ClassPredictor -> mask branch -> the mask column of each box's
        PREDICTED class (roi.mask_predict).  Needs a step built with class_loss=True (the class branch exists only then).
        -> dict with the reference's keys in the reference's spelling: `roi_bbox` (list of [n_s, 2, 3]), `class` (list of
        int64 [n_s]), `class_propabilities` (list of [n_s, 18]), `mask` (list of fp32 [n_s, N_s]), and, when the step has the
        segmentation head, `segmentation_class` (int64 [N]) / `segmentation_probabilites` ([N, 20])."""
        if self.model.class_branch is None:
            raise ValueError("predict() needs the class branch: build the step with class_loss=True")
        from . import roi
        run = self._infer(k, with_class=True)
        class_scores, _, (class_indices, class_prob, class_raw) = run["class"]
        logits, (sel, counts, splits) = run["logits"], run["selection"]
        with torch.no_grad():
            masks = roi.mask_predict(logits, sel, counts, splits, class_raw)
            result = {"roi_bbox": run["boxes"], "class": list(class_indices), "class_propabilities": list(class_prob), "mask": masks}
            if self.model.segmentation is not None:
                _, (result["segmentation_class"], result["segmentation_probabilites"]) = self._infer_segmentation(run["out"])
        self.predict_out = (class_scores, logits, (sel, counts, splits))       # (for checks)
        return result

    def evaluate(self, scenes=None, *, score_threshold=0.9, mask_threshold=0.5, overlap_thresholds=(0.25, 0.5), eval_on_gt=True):
        """The reference's `eval_model` (training.py:98-304; defaults scannet_config/run.py:917-934) on the step's own scenes
        (`scenes`: micro-batch indices, default all): per micro-batch the chain of `predict()` under torch.no_grad(), but the
        masks go logits -> packed bits -> popcount IoU (evaluation.mask_bits / mask_iou) and never exist as dense fp32;
        `roi_score` is the ROI selector's.  With `eval_on_gt` the class branch and the mask branch also run on the ground-truth
        boxes (model.py:194-238) and fill `gtbbox`, `gtmask`, `gtlabelmask`; the segmentation head, if the step has one, fills
        `segment`.  Needs a step built with class_loss=True.  -> (combined_metrics, single_class_metrics) with the reference's
        keys, `gtbbox_AP*` dropped as training.py:174-177 does; the accumulators stay on `self.eval_out`.  The metrics wait for
        the host once per overlap accumulator and once per confusion accumulator; the forward waits where predict() does.
        `scenes` may name the micro-batches in any order: the index structures are built by the forward itself, and an index
        build that a previous step() prefetched is joined and dropped (the next step builds its own)."""
        m = self.model
        if m.class_branch is None:
            raise ValueError("evaluate() needs the class branch: build the step with class_loss=True")
        from . import evaluation as E
        from .loss import pack_gt_masks
        k_cls = m.mask.classes
        bbox_calc = E.BboxOverlapCalculator(score_threshold=score_threshold)
        mask_calc = E.MaskOverlapCalculator(mask_threshold, score_threshold=score_threshold)
        names = ["bbox", "mask"] + (["gtbbox", "gtmask", "gtlabelmask"] if eval_on_gt else [])
        acc = {n: E.OverlapAccumulator(bbox_calc if "bbox" in n else mask_calc) for n in names}
        label_acc = E.ConfusionAccumulator(E.ConfusionCalculator(k_cls))
        bin_acc = E.BinaryConfusionAccumulator(E.BinaryMaskConfusionCalculator(mask_threshold))
        seg_acc = None
        for k in (range(self.batches_per_step) if scenes is None else scenes):
            sc = self._scenes[k]
            gt_boxes, gt_label = sc["gt_dev"], sc["gt_label"]
            run = self._infer(k, with_class=True, classify_too=gt_boxes if eval_on_gt else None, own_index=True)
            out, roi_score, boxes = run["out"], run["roi_score"], run["boxes"]
            _, _, (class_indices, _, class_raw) = run["class"]
            logits, (sel, counts, splits) = run["logits"], run["selection"]
            with torch.no_grad():
                pred_bits = E.mask_bits(logits, sel, counts, splits, class_raw, 0, mask_threshold)
                if "gt_mask" not in sc:
                    sc["gt_mask"] = pack_gt_masks([mk.to(self.device) for mk in sc["gt_mask_cpu"]])
                gt_mask = sc["gt_mask"]
                acc["bbox"].add_batch(roi_score, boxes, gt_boxes, list(class_indices), gt_label)
                acc["mask"].add_batch(roi_score, pred_bits, gt_mask, list(class_indices), gt_label)
                if eval_on_gt:                 # model.py:194-238: the same two branches on the ground-truth boxes
                    _, _, (gt_class, _, gt_class_raw) = run["class_too"]
                    pseudo = [b.new_ones((len(b),)) for b in gt_boxes]
                    glogits, (gsel, gcounts, gsplits) = self._infer_mask(out, gt_boxes)
                    gt_bits = E.mask_bits(glogits, gsel, gcounts, gsplits, gt_class_raw, 0, mask_threshold)
                    gtl_bits = E.mask_bits(glogits, gsel, gcounts, gsplits, torch.cat(list(gt_label)), 0, mask_threshold)
                    acc["gtbbox"].add_batch(pseudo, gt_boxes, gt_boxes, list(gt_class), gt_label)
                    label_acc.add_list_batch(list(gt_class), gt_label)
                    acc["gtmask"].add_batch(pseudo, gt_bits, gt_mask, list(gt_class), gt_label)
                    acc["gtlabelmask"].add_batch(pseudo, gtl_bits, gt_mask, gt_label, gt_label)
                    bin_acc.add_batch(gtl_bits, gt_mask, gt_boxes, gt_label)
                if m.segmentation is not None and "seg_target" in sc:
                    seg_logits, (seg_class, _) = self._infer_segmentation(out)
                    if seg_acc is None:
                        seg_acc = E.ConfusionAccumulator(E.ConfusionCalculator(int(seg_logits.shape[1])))
                    seg_acc.add_batch(seg_class, sc["seg_target"])
        helper = E.EvaluationHelper(list(overlap_thresholds), list(range(k_cls)))
        combined, single_class, _, conf, oconf, binary = helper(
            acc, {"segment": seg_acc} if seg_acc is not None else {}, {"gtbbox": label_acc} if eval_on_gt else {},
            {"gtlabelmask": bin_acc} if eval_on_gt else {})
        combined = {key: v for key, v in combined.items() if "gtbbox_AP" not in key}
        self.eval_out = dict(overlap=acc, segment=seg_acc, gtbbox=label_acc if eval_on_gt else None,
                             gtlabelmask=bin_acc if eval_on_gt else None, confusion=conf, overlap_confusion=oconf, binary=binary)
        return combined, single_class

    def step(self):
        n = self.batches_per_step
        for k in range(n - 1):                    # training.py:436: (loss / batches_per_step).backward(), no update yet
            with self.flat.accumulate():
                self.forward_backward(k, zero=(k == 0))
        self.forward_backward(n - 1, zero=(n == 1))       # the last micro-batch: bucket hooks armed, slices go out
        if self.adam is not None:
            self.adam.lr = self.lr
        if self.weighting == "count":
            self.flat.all_reduce_mean(total_weight=self._total_weight)
            if self.adam is not None:
                self.flat.adam_step(self.adam)
            else:
                self.flat.sgd_step(self.lr)
        elif self.adam is not None:
            self.flat.adam_step_single_rank(self.adam)
        else:
            self.flat.step_single_rank(self.lr)  # = all_reduce_mean + sgd_step; one rank: no packing into the flat bucket

    @property
    def max_grad_norm(self):
        """The bound the step clips its gradient to (None: no clipping), as given at construction."""
        return self._max_grad_norm

    @property
    def grad_norm(self):
        """(total_norm, clip_coef, nonfinite) of the last step's clip, read from the device record on access (the step's only host
        wait for it); None without max_grad_norm or before the first step."""
        rec = self.flat.clip_record
        if self.max_grad_norm is None or rec is None:
            return None
        total, coef, bad = rec[:3].tolist()
        return total, coef, bool(bad)

    def finish(self):
        """Join the index build started by the last step (it belongs to the timed region)."""
        if self._md_next is not None:
            self._md_next.result()
            self._md_next = None

    def describe(self):
        return "".join((self._describe_backbone(), self._describe_boxes(), self._describe_losses(), self._describe_stages(),
                        self._describe_container(), self._describe_accumulation(), self._describe_optimizer(),
                        self._describe_tail()))

    # ---- describe(), section by section --------------------------------------------------------------------------------
    def _describe_backbone(self):
        units = ", 2 pre-act residual blocks/level"
        if self.bottleneck_divisor or self.main_path_relu:
            units = (", 2 residual units/level (" + ", ".join(
                ([f"bottleneck_divisor={self.bottleneck_divisor}"] if self.bottleneck_divisor else [])
                + (["main_path_relu=True"] if self.main_path_relu else [])) + ")")
        stages = ""
        if not (self.relu_first and self.drop_input_relu and self.use_residuals):
            stages = " (" + ", ".join(
                ([] if self.relu_first else ["relu_first=False: post-activation units, layer -> ReLU input stages"])
                + ([] if self.drop_input_relu else ["drop_input_relu=False"])
                + ([] if self.use_residuals else ["use_residuals=False: plain convolution blocks"])) + ")"
        bn = ""
        if self.workload.endswith("-bn"):
            bn = (", BatchNormReLU in the residual units (training mode, fp64 statistics; "
                  + ("step-executor stages, one node per level)" if self.model.backbone.unet._bn_staged() else "layer-by-layer path)"))
        return (f"BASELINE {self.baseline_entry}: {self.batch_size} " + ("converted sample(s) per GPU (sample.convert_sample + collate),"
                if self.from_batches else "synthetic ScanNet-shaped sample(s) per GPU,") + f" {self.n_active} "
                f"active voxels (grid {self.grid[0]}x{self.grid[1]}x{self.grid[2]}, 1.15 points/voxel), U-Net "
                + "-".join(map(str, self.channels)) + units + ", 2^3/2 conv+deconv" + stages + bn)

    def _describe_boxes(self):
        """The RPN, the proposal selection, the crop and the mask branch."""
        if not self.n_boxes:
            return ""
        if not self.with_rpn:
            return (f"; + {self.n_boxes} fp32 boxes/scene (edges 8-96 voxels) -> sparse ROI crop ({self.n_roi_rows} cropped "
                    "points) -> mask branch (SubM1 + 2 units @16, internal U-Net 23-32-48-64, Linear 23-32-18); CROP + MASK "
                    "BRANCH ONLY: the boxes are synthetic and known before the forward (no RPN in this step; "
                    "--workload cfg3-rpn has it)")
        r = self.model.rpn
        sel = (f"-> anchors that leave the scene dropped (anchor.py:103-113) -> sigmoid, top-1024, boxes clipped to the scene, "
               f"one-launch NMS 0.5, <= {self.n_boxes} boxes/sample" + (f", the {self.mask_boxes} best of them per sample" if self.mask_boxes else "")
               + f" -> sparse ROI crop ({self.n_roi_rows} cropped points) -> mask "
               "branch (SubM1 + 2 units @16, internal U-Net 23-32-48-64, Linear 23-32-18); backward from the backbone "
               "output, rpn_bbox, rpn_score and the mask logits")
        if hasattr(r, "levels"):
            return self._describe_reference_rpn(r) + sel
        eng = r.engine or r.ENGINE
        return (f"; + RPN boundary INSIDE the step, a STAND-IN lighter than the reference's (one anchor level, 2 x {r.width} "
                f"stack, {self.n_boxes} kept; the reference: two levels, 5 x 128 / 5 x 256, 256 kept -- `ref-crop-rpn`): "
                f"SparseToDense of the stride-{r.stride} level ({r.channels} ch) -> dense dilation stack {r.channels}"
                + f"-{r.width}" * (len(r.stack) // 2) + f" (3^3, engine '{eng}': "
                + ("this library's tile kernels on a fully active grid" if eng == "tiles" else "torch / MIOpen conv3d")
                + f") + 1x1 head ({r.n_anchors} anchors/cell) " + sel)

    def _describe_reference_rpn(self, r):
        eng = r.levels[0].engine or r.levels[0].ENGINE
        up = getattr(r, "anchor_network", None)

        def head(i, l):
            if up is None:
                return f"1x1 head ({l.n_anchors} anchors/cell)"
            return ("up-sampling heads (" + ", ".join("x".join(map(str, g["extra"])) + f": {g['n_anchors']}"
                                                      for g in up._groups[i]) + " anchors per fine cell)")
        return ("; + the REFERENCE's RPN shape INSIDE the step (run.py:525-536,609,847-853): " + " + ".join(
            f"SparseToDense of the stride-{l.stride} level ({l.channels} ch) -> dense dilation stack {l.channels}"
            + f"-{l.width}" * (len(l.stack) // 2) + " (3^3) + " + head(i, l) for i, l in enumerate(r.levels))
            + f", dense layers on engine '{eng}' "
            + ("(this library's tile kernels on a fully active grid)" if eng == "tiles" else "(torch / MIOpen conv3d)")
            + ("; 1x1 heads (AnchorNetworkConv), every anchor on its level's own grid -- the reference's committed "
               "AnchorNetworkUpsample heads: upsample_heads=True " if up is None else
               "; the reference's AnchorNetworkUpsample heads (run.py:339,532-537): per level one transposed "
               "convolution with kernel = stride per group of anchors, as one row GEMM + one scatter "
               "(scn_anchor_up.hip)"
               + (", behind a bf16-STORED stack whose last ReLU runs on the bf16 slab (scn_relu_fwd_bf16 / _bwd_bf16); "
                  "the heads' row GEMM, P, the scatter and rpn_bbox / rpn_score are fp32 "
                  if self.dtype == "bf16" else " ")))

    def _describe_losses(self):
        s = ""
        if self.rpn_loss:
            s += ("; the RPN trains on the reference's RPN loss (BCE-with-logits + smooth L1, sigma 2) against the synthetic "
                  "boxes: device anchor targets, batch-wide 0.35 / 0.15 sampling, max weight 1/8 (scn_rpnloss.hip)")
        if self.mask_loss:
            s += ("; the mask branch trains on the reference's mask loss: IoU of the proposals against the synthetic ground "
                  "truth" + (f" (the first {self.n_gt} boxes per sample)" if self.n_gt else "") + ", TrainSelector(0.2, 0, "
                  "(24, 0, True)) draws <= 24 proposals with IoU >= 0.2 per sample and appends every ground-truth box "
                  "(one launch), BCE-with-logits of the instance's label column against its ellipsoid mask, mean over the "
                  "boxes with points (scn_maskloss.hip)")
        elif self.n_gt:
            s += f"; ground truth: the first {self.n_gt} synthetic boxes per sample"
        if self.class_loss:
            s += self._describe_class_branch()
            s += ("TrainSelector(0.1, 0, (32, 0, True)) draws <= 32 proposals with IoU >= 0.1 per sample and appends every "
                  "ground-truth box, cross entropy against the associated instance's label (scn_xent.hip)")
        if self.segmentation_loss:
            s += ("; the segmentation head (SubM 1^3 to 20 classes, one row per point) trains on the reference's segmentation "
                  "loss: cross entropy against the instances' labels + 2, -100 (ignored) outside every instance; its gradient "
                  "replaces the synthetic one at the backbone output (scn_xent.hip)")
        return s

    def _describe_class_branch(self):
        cb = self.model.class_branch
        if self.simple_class:
            return ("; the RESHAPING class head of the dense arm (`simple_class`: no input convolution; RoiAlign to " +
                    "x".join(map(str, cb.cut_shape)) + " and max pool 2 in one pass out of the stride-" + str(cb.stride) +
                    " volume of the RPN's dilation stack at its full width (scn_roialign_pool_fwd / _bwd" +
                    ("" if cb.fused else ": OFF, the two-call pair") + "), " +
                    ", ".join(f"3^3 same-conv {m.nIn}->{m.nOut}" for m in cb.output_conv_layer) + " on fully active box grids, "
                    "channel-major flatten, Linear " + "-".join(str(m.in_features) for m in cb.linear_layer
                                                                 if isinstance(m, torch.nn.Linear)) + f"-{cb.num_classes}, fp32"
                    ") trains the stack too, on the reference's class loss: ")
        if self.dense_class:
            return ("; the DENSE class branch (1^3 conv + 1 unit @32 on the stride-" + str(cb.stride) + " volume of the RPN's dilation "
                    "stack, RoiAlign to " + "x".join(map(str, cb.cut_shape)) + " (scn_roialign.hip), max pool 2 without clamp, "
                    "2^3/2 conv + unit @64 and @128 on fully active box grids, mean pool, Linear 128-64-18" +
                    (", its slabs bf16-STORED from the stack's stored volume to the mean pool (class_storage bf16: "
                     "scn_roialign_fwd_bf16 / scn_dense_maxpool_fwd_bf16, fp32 accumulation, fp32 linear layers)"
                     if self.class_storage else "") + ") trains the stack too, "
                    "on the reference's class loss: ")
        return ("; the class branch (SubM1 + 1 unit @32 on the stride-" + str(cb.stride) + " level, sparse "
                "ROI cut, 2^3/2 conv + unit @64 and @128, mean pool, Linear 128-64-18) trains on the reference's class loss: ")

    def _describe_stages(self):
        s = ""
        if self.train is not None:
            s += ("; TRAINING IN STAGES (train=" + repr(self.train) + "; the reference's mask_only / unet_tweak, run.py:332,"
                  "1414-1427): trainable parts " + ", ".join(self.trainable) + "; frozen parts "
                  + (", ".join(self.frozen) or "none") + " (requires_grad False, outside the flat buffer and the optimizer, "
                  "forward-only where nothing trainable lies below them); requested losses not computed: "
                  + (", ".join(self.losses_not_computed) or "none")
                  + " (no targets, draws or selector launches, the head not run in the step; predict() / evaluate() run it)")
        if self.init_missing is not None:
            s += (f"; initialised from an earlier stage's state_dict (init_state, the reference's ignore_load): "
                  f"{len(self.init_missing)} model keys kept their own initialisation, {len(self.init_unused)} keys of the dict unused")
        return s

    def _describe_container(self):
        return "" if self.combiner is None else (
                "; the losses are combined by the reference's loss container (loss.LossCombiner: loss = sum of term x "
                "exp(-log-weight) + the log-weights, the two RPN weights crossed as in loss.py:111-114; "
                + ("multitask_loss: the five log-weights are parameters in the flat buffer" if self.multitask_loss
                   else "fixed weights " + ", ".join(f"{k} {v:g}" for k, v in self._loss_weights.items()))
                + "): one scn_loss_combine launch per micro-batch between forward and backward writes the roots' gradients"
                + (" and adds the log-weights' gradients into the flat gradient buffer" if self.multitask_loss else "")
                + " (scn_xent.hip)")

    def _describe_accumulation(self):
        return "" if self.batches_per_step == 1 else (
            f"; {self.batches_per_step} micro-batches (scenes) accumulated per optimizer step (training.py:436,458-460), "
            "voxels = all of them")

    def _describe_clip(self):
        if self.max_grad_norm is None:
            return ""
        from .executor import clip_launches
        # (step(): the count-weighted step reduces explicitly; otherwise FlatParams decides between the packed and the fast path)
        packed = self.weighting == "count" or self.flat.single_rank_step_packs()
        n = [self.flat.flat.numel()] if packed else [p.numel() for p in self.flat.params]
        return (f"; the gradient the update reads is clipped to the L2 norm {self.max_grad_norm:g} on the device before it "
                "(SCN_OP_GRAD_NORM + SCN_OP_GRAD_SCALE in one executor call, scn_clip.hip: sum of squares in double, fixed order, "
                f"torch's fp32 coefficient, no host wait; {clip_launches(n)} launches per step over "
                + ("the packed flat gradient" if packed else f"the {len(n)} gradient tensors where autograd left them, one rank")
                + "; `.grad_norm` reads the step's own record)")

    def _describe_optimizer(self):
        if self.adam is not None:
            a = self.adam
            return (f"; step = rulebooks + fwd + bwd (+ grad all-reduce) + Adam (the reference's optimizer, scannet_config/run.py:"
                    f"1449) on the flat parameter buffer, lr {self.lr:g}, betas ({a.betas[0]:g}, {a.betas[1]:g}), eps {a.eps:g}, "
                    f"weight decay {a.weight_decay:g}: one fused update launch per <= 80 tensors" + self._describe_clip())
        return (f"; step = rulebooks + fwd + bwd (+ grad all-reduce) + plain SGD on the flat parameter buffer, lr {self.lr:g} "
                "(the reference trains with Adam, scannet_config/run.py:1449: three more passes over the buffer)"
                + self._describe_clip())

    def _describe_tail(self):
        s = ""
        if self.step_group and not self.flat.buckets and self.dtype == "f32" and self.batches_per_step == 1:
            s += ("; fp32 weight gradients of the whole step in one grid per kernel variant after the last backward pass "
                  "(workspaces and unit slabs live until then; step_group=False: per pass)")
        if self.prefetch:
            s += "; rulebooks of batch i+1 built on a helper thread during batch i"
        return s