"""Graph builders for the reference's class branch and segmentation head.

``ClassBranch``: the topology the reference's sparse ``ClassNetwork`` (ndsis/modules/model.py:470-569) has under
scannet_config/run.py:633-732 (the `sparse and not class_output_anchor` arm), expressed with this package's modules:

  feature map (C ch at `stride`, one row per active site of the coarsest RPN level)
    -> input_conv_layer   : 'B' level, 32 ch, stride 1: SubM 1^3 C->32 + 1 residual unit              (run.py:659-669)
    -> roi_getter         : SparseRoiCut(TensorToTensor, clip_boxes=True, resize_boxes=stride): the sites inside each
                            box (scene units / stride, clipped to the grid), InputLayer mode 0, batch_size = #boxes
    -> output_conv_layer  : Convolution 32->64 2^3/2 + unit, Convolution 64->128 2^3/2 + unit          (run.py:681-696)
    -> vectorice_layer    : SparseGlobalPool(torch.mean): one row per box, zeros for a box without sites
    -> linear_layer       : ReLU, Linear(128, 64), ReLU, Linear(64, num_classes)                       (run.py:723-728)

``DenseClassBranch``: the same ClassNetwork on its DENSE arm, the one the reference's committed configuration takes
(scannet_config/run.py:340 `dense_class = True`, so `class_output_anchor=True` :603 and `cut_shape = (16, 16, 16)` :636-638): it
reads the dense volume an anchor level's dilation stack produced (model.py:435-437), here the channels-last slab
rpn.DenseRpn keeps:

  volume slab [B X Y Z, C] (the fully active grid of the anchor level)
    -> input_conv_layer   : 1^3 C->32 + 1 residual unit on the whole volume
    -> roi_getter         : roi.RoiAlign(cut_shape, clip_boxes=True, resize_boxes=stride): every box trilinear to 16^3
                            (scn_roialign_fwd) -- the slab of the fully active grid 16^3 with batch R
    -> dense max pool 2   : the plain maximum, no clamp (scn_dense_maxpool_fwd; scn.MaxPooling clamps at 0)
    -> output_conv_layer  : Convolution 32->64 2^3/2 + unit, Convolution 64->128 2^3/2 + unit on the fully active box grids
                            8^3, 4^3, 2^3 -- a dense same-convolution is a submanifold convolution on a fully active grid (rpn.py)
    -> vectorice_layer    : mean over the 2^3 sites of a box
    -> linear_layer       : ReLU, Linear(128, 64), ReLU, Linear(64, num_classes)

``SegmentationHead``: the reference's sparse ``SegmentationNetwork`` (model.py:449-467): SubM 1^3 C->num_classes with
bias, then the OutputLayer: one row of class scores per point.
"""
from __future__ import annotations

import torch
from torch import nn

from . import modules as M
from . import roi
from .custom_operations import SparseGlobalPool
from .ioLayers import OutputLayer
from .unet import units


def reference_key_map(n_output_levels=2, num_units=1, n_linear=2):
    """state_dict key of the reference's ClassNetwork -> this package's parameter name (`ClassBranch.named_oracle_params`).
    Checked against the key list of a reference ClassNetwork built on this package (tests/golden/dropin_class_network.json)."""
    out = {}
    for t in ("weight", "bias"):
        out[f"input_conv_layer.0.0.0.{t}"] = f"in.{t}"
        for u in range(num_units):
            for v, idx in enumerate((1, 3)):                     # Sequential(ReLU, SubM, ReLU, SubM) inside ConcatTable[1]
                out[f"input_conv_layer.0.1.{u}.0.1.{idx}.{t}"] = f"in.res{u}.conv{v}.{t}"
        for l in range(n_output_levels):
            out[f"output_conv_layer.{l}.0.0.{t}"] = f"down{l}.{t}"
            for u in range(num_units):
                for v, idx in enumerate((1, 3)):
                    out[f"output_conv_layer.{l}.1.{u}.0.1.{idx}.{t}"] = f"down{l}.res{u}.conv{v}.{t}"
        for i in range(n_linear):
            out[f"linear_layer.{2 * i + 1}.{t}"] = f"lin{i}.{t}"      # ReLU, Linear, ReLU, Linear: indices 1, 3
    return out


def _load_mapped(own, kmap, state_dict, prefix, mine, strict):
    missing, used = [], set()
    with torch.no_grad():
        for rk, name in kmap.items():
            t = state_dict.get(prefix + rk)
            if t is None:
                missing.append(prefix + rk)
                continue
            if t.dim() == 4 and t.shape[1] == 1:                 # SparseConvNet's grouped layout [fv, 1, nIn, nOut]
                t = t.squeeze(1)
            p = own[name]
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"{prefix + rk}: checkpoint shape {tuple(t.shape)} != {tuple(p.shape)} ({name})")
            p.copy_(t)
            used.add(prefix + rk)
    unused = [k for k in state_dict if k.startswith(prefix) and k[len(prefix):].startswith(mine) and k not in used]
    if strict and (missing or unused):
        raise KeyError(f"reference checkpoint mismatch: missing {missing[:4]}... unused {unused[:4]}...")
    return missing, unused


def _unit_convs(block):
    return [m for m in block[0][1] if isinstance(m, M.SubmanifoldConvolution)]


class ClassBranch(nn.Module):
    """forward(feature_map, boxes) -> (class_scores [BB, num_classes] fp32, selection = (RoiSelection, boxes per sample,
    sites per sample)).  feature_map: SparseConvNetTensor of `feature_channels` channels whose sites are `stride` scene units
    apart; boxes: list (one per sample) of fp32 [n, 2, 3] (start, stop) boxes in scene units (training: TrainSelector's
    forward boxes; evaluation: the kept proposals).  A box without any site pools to a zero row: its scores are the Linear
    stack's bias response, finite, and it adds nothing to the convolutions' gradients.
    The branch computes in fp32: a bf16-stored feature map is widened once on entry, and the branch's own layers keep fp32
    rows whatever `set_feature_storage` says (the ROI batch is a few thousand rows)."""

    def __init__(self, feature_channels, stride, input_channels=32, output_channels=(64, 128), linear_channels=(64,),
                 num_classes=18, num_units=1):
        super().__init__()
        self.stride, self.num_units = int(stride), int(num_units)
        self.input_conv_layer = M.Sequential(M.SubmanifoldConvolution(3, feature_channels, input_channels, 1, True),
                                             units(input_channels, num_units))
        self.roi_getter = roi.SparseRoiCut(roi.TensorToTensorFeatureExtractorCombiner(), clip_boxes=True,
                                           resize_boxes=self.stride, dense_inside=False)
        levels, c = [], input_channels
        for co in output_channels:
            levels.append(M.Sequential(M.Convolution(3, c, co, 2, 2, True), units(co, num_units)))
            c = co
        self.output_conv_layer = M.Sequential(*levels)
        self.vectorice_layer = SparseGlobalPool(torch.mean)
        layers = []
        for co in tuple(linear_channels) + (num_classes,):
            layers += [nn.ReLU(inplace=bool(layers)), nn.Linear(c, co)]
            c = co
        self.linear_layer = nn.Sequential(*layers)
        self.pooled_channels = tuple(output_channels)[-1] if len(output_channels) else input_channels
        self.num_classes = int(num_classes)

    def forward(self, feature_map, boxes):
        prev = M.set_feature_storage(torch.float32)
        try:
            if feature_map.features.dtype != torch.float32:
                feature_map = M.CastFeatures(torch.float32)(feature_map)
            augmented = self.input_conv_layer(feature_map)
            box_features, selection = self.roi_getter(augmented, boxes)
            n_boxes = sum(int(c) for c in selection[1])
            if box_features is None:                             # no box holds a site: every pooled row is zero
                pooled = augmented.features.new_zeros((n_boxes, self.pooled_channels))
            else:
                pooled = self.vectorice_layer(self.output_conv_layer(box_features))
        finally:
            M.set_feature_storage(prev)
        return self._linear(pooled), selection

    def _linear(self, x):
        """The ReLU / Linear stack (module_factory.py:700-716) on the library's row GEMM, as MaskBranch._linear."""
        from . import functional as F
        for m in self.linear_layer:
            if isinstance(m, nn.Linear):
                x = F.NetworkInNetworkFunction.apply(x, m.weight.t(), m.bias)
            else:
                x = F.ReLUFunction.apply(x)
        return x

    def named_oracle_params(self):
        out = {}
        ic = self.input_conv_layer
        out["in.weight"], out["in.bias"] = ic[0].weight, ic[0].bias
        for u, block in enumerate(ic[1]):
            for v, cv in enumerate(_unit_convs(block)):
                out[f"in.res{u}.conv{v}.weight"], out[f"in.res{u}.conv{v}.bias"] = cv.weight, cv.bias
        for l, level in enumerate(self.output_conv_layer):
            out[f"down{l}.weight"], out[f"down{l}.bias"] = level[0].weight, level[0].bias
            for u, block in enumerate(level[1]):
                for v, cv in enumerate(_unit_convs(block)):
                    out[f"down{l}.res{u}.conv{v}.weight"], out[f"down{l}.res{u}.conv{v}.bias"] = cv.weight, cv.bias
        for i, m in enumerate(m for m in self.linear_layer if isinstance(m, nn.Linear)):
            out[f"lin{i}.weight"], out[f"lin{i}.bias"] = m.weight, m.bias
        return out

    def reference_key_map(self):
        n_lin = len([m for m in self.linear_layer if isinstance(m, nn.Linear)])
        return reference_key_map(len(self.output_conv_layer), self.num_units, n_lin)

    def load_reference_state_dict(self, state_dict, prefix=None, strict=True):
        """Load the class-network part of a checkpoint written by the REFERENCE (the ClassNetwork sits under `class_network.`
        in InstanceSegmentationNetwork, model.py:31-114).  prefix=None: detected from the first key ending in
        'input_conv_layer.0.0.0.weight' that has a 'linear_layer.1.weight' sibling (the mask network has none).
        -> (missing reference keys, unused checkpoint keys under the prefix)."""
        if prefix is None:
            tail = "input_conv_layer.0.0.0.weight"
            cands = [k[:-len(tail)] for k in state_dict if k.endswith(tail)]
            prefix = next((c for c in cands if c + "linear_layer.1.weight" in state_dict), cands[0] if cands else "")
        return _load_mapped(self.named_oracle_params(), self.reference_key_map(), state_dict, prefix,
                            ("input_conv_layer.", "output_conv_layer.", "linear_layer."), strict)


def dense_reference_key_map(n_output_levels=2, num_units=1, n_linear=2):
    """state_dict key of the reference's DENSE ClassNetwork -> this package's parameter name
    (`DenseClassBranch.named_oracle_params`).  The dense residual is a `DenseResidual` whose convolutions sit at
    `inner_block.{1,3}`; index 0 of `output_conv_layer` is the parameterless max pool, so level l sits at l + 1.  Checked against
    the key lists of reference networks built on the CPU (tests/golden/dense_class_keys.json)."""
    out = {}
    for t in ("weight", "bias"):
        out[f"input_conv_layer.0.0.0.{t}"] = f"in.{t}"
        for u in range(num_units):
            for v, idx in enumerate((1, 3)):
                out[f"input_conv_layer.0.1.{u}.inner_block.{idx}.{t}"] = f"in.res{u}.conv{v}.{t}"
        for l in range(n_output_levels):
            out[f"output_conv_layer.{l + 1}.0.0.{t}"] = f"down{l}.{t}"
            for u in range(num_units):
                for v, idx in enumerate((1, 3)):
                    out[f"output_conv_layer.{l + 1}.1.{u}.inner_block.{idx}.{t}"] = f"down{l}.res{u}.conv{v}.{t}"
        for i in range(n_linear):
            out[f"linear_layer.{2 * i + 1}.{t}"] = f"lin{i}.{t}"
    return out


def conv3d_to_slab_weight(w):
    """nn.Conv3d weight [co, ci, a, b, c] -> this package's W[(a K + b) K + c, ci, co] (rpn.py; K = 1, 2 or 3)."""
    co, ci = w.shape[:2]
    return w.permute(2, 3, 4, 1, 0).reshape(-1, ci, co)


def slab_to_conv3d_weight(W, k):
    """The inverse of `conv3d_to_slab_weight` for a K^3 kernel."""
    _, ci, co = W.shape
    return W.reshape(k, k, k, ci, co).permute(4, 3, 0, 1, 2)


BOX_BUCKET = 32


class DenseClassBranch(nn.Module):
    """forward(volume_slab [B X Y Z, feature_channels], size (X, Y, Z), batch, boxes) -> (class_scores [R, num_classes] fp32,
    (bbox_tensor [R, 2, 3] in cells, boxes per sample, size)): the middle entry is what ClassLossSelector / ClassPredictor read.
    boxes: list (one per sample) of fp32 [n, 2, 3] (start, stop) boxes in scene units; `stride` scene units per cell.
    storage=torch.float32 (default): the branch computes in fp32, as ClassBranch does -- a bf16 volume is widened on entry.
    storage=torch.bfloat16: the branch's slabs are bf16-STORED -- a bf16 volume is used as it is (an fp32 one is cast once: exact
    when the RPN stack stored bf16), the input convolution, RoiAlign (scn_roialign_fwd_bf16), the max pool and the strided levels
    run on bf16 slabs under `set_feature_storage(torch.bfloat16)` with fp32 accumulation, SparseGlobalPool widens the final rows,
    and the linear layers and the scores are fp32.  Parameters, their gradients and the checkpoint maps do not change.  Every
    width (feature_channels, input_channels, output_channels) must then be a multiple of 8, the bf16 lane.

    The box count changes every training step and the index structures of a fully active grid depend on its batch, so R is
    rounded up to a multiple of BOX_BUCKET and ONE Metadata is kept per bucket: the padding boxes' rows enter the first strided
    convolution as zeros (functional.DenseMaxPoolFunction writes them), their pooled rows are dropped before the linear
    layers, so their output gradient is zero and they add nothing to any weight gradient; boxes never share a site, so
    they change no real box's result.

    fused_pool=True (opt-in; the default path is unchanged): RoiAlign and the max pool run as ONE pass
    (functional.RoiAlignPoolFunction, in either storage) -- the same scores bit for bit, the [R 16^3, C] samples never written."""

    def __init__(self, feature_channels, stride, input_channels=32, output_channels=(64, 128), linear_channels=(64,),
                 num_classes=18, num_units=1, cut_shape=(16, 16, 16), storage=torch.float32, fused_pool=False):
        super().__init__()
        self.fused_pool = bool(fused_pool)
        if storage not in (torch.float32, torch.bfloat16):
            raise ValueError("DenseClassBranch: storage is torch.float32 or torch.bfloat16")
        widths = (feature_channels, input_channels) + tuple(output_channels)
        if storage is torch.bfloat16 and any(int(w) % 8 for w in widths):
            raise ValueError(f"DenseClassBranch(storage=torch.bfloat16): every width must be a multiple of 8 (16-byte lanes of "
                             f"bf16 rows), got feature / input / output channels {widths}")
        self.storage = storage
        self.stride, self.num_units = stride, int(num_units)
        self.cut_shape = tuple(int(c) for c in cut_shape)
        down = 2 ** (1 + len(output_channels))
        if any(c % down or c < down for c in self.cut_shape):
            raise ValueError(f"DenseClassBranch: cut_shape {self.cut_shape} must be a multiple of {down} (max pool 2 and "
                             f"{len(output_channels)} 2^3/2 convolutions)")
        self.input_conv_layer = M.Sequential(M.SubmanifoldConvolution(3, feature_channels, input_channels, 1, True),
                                             units(input_channels, num_units))
        self.roi_getter = roi.RoiAlign(self.cut_shape, clip_boxes=True, resize_boxes=stride)
        levels, c = [], input_channels
        for co in output_channels:
            levels.append(M.Sequential(M.Convolution(3, c, co, 2, 2, True), units(co, num_units)))
            c = co
        self.output_conv_layer = M.Sequential(*levels)
        self.vectorice_layer = SparseGlobalPool(torch.mean)
        layers = []
        for co in tuple(linear_channels) + (num_classes,):
            layers += [nn.ReLU(inplace=bool(layers)), nn.Linear(c, co)]
            c = co
        self.linear_layer = nn.Sequential(*layers)
        self.num_classes = int(num_classes)
        self._md = {}                         # (kind, size, batch, device) -> fully active Metadata

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_md"] = {}
        return d

    def _metadata(self, size, batch, device):
        from .rpn import fully_active_metadata
        key = (tuple(int(v) for v in size), int(batch), str(device))
        md = self._md.get(key)
        if md is None:
            md = self._md[key] = fully_active_metadata(key[0], key[1], device)
        return md

    @staticmethod
    def bucket(n_boxes):
        return -(-int(n_boxes) // BOX_BUCKET) * BOX_BUCKET

    def forward(self, volume_slab, size, batch, boxes, metadata=None):
        """metadata: the volume's fully active Metadata if the caller has it (DenseRpn.volume[3]); else built once and kept."""
        from . import functional as F
        from .tensor import SparseConvNetTensor
        size = tuple(int(v) for v in size)
        prev = M.set_feature_storage(self.storage)
        try:
            if volume_slab.dtype != self.storage:
                volume_slab = volume_slab.to(self.storage)
            md = metadata if metadata is not None else self._metadata(size, batch, volume_slab.device)
            augmented = self.input_conv_layer(SparseConvNetTensor(volume_slab, md, torch.as_tensor(size, dtype=torch.long)))
            if self.fused_pool:
                bbox_tensor, counts, assoc = roi.transform_boxes_interpolation(boxes, size, True, self.stride)
                selection = (bbox_tensor, counts, size)
            else:
                box_slab, selection = self.roi_getter.forward_slab(augmented.features, size, batch, boxes)
            r = selection[0].shape[0]
            if r == 0:
                return volume_slab.new_zeros((0, self.num_classes), dtype=torch.float32), selection
            rb = self.bucket(r)
            half = tuple(c // 2 for c in self.cut_shape)
            if self.fused_pool:
                sample = assoc.to(device=volume_slab.device, dtype=torch.int32)
                pooled = F.RoiAlignPoolFunction.apply(augmented.features, selection[0], sample, int(batch), size,
                                                      self.cut_shape, rb)
            else:
                pooled = F.DenseMaxPoolFunction.apply(box_slab, r, self.cut_shape, rb)
            box_md = self._metadata(half, rb, volume_slab.device)
            x = SparseConvNetTensor(pooled, box_md, torch.as_tensor(half, dtype=torch.long))
            vectors = self.vectorice_layer(self.output_conv_layer(x))[:r]
        finally:
            M.set_feature_storage(prev)
        return self._linear(vectors), selection

    _linear = ClassBranch._linear
    named_oracle_params = ClassBranch.named_oracle_params

    def reference_key_map(self):
        n_lin = len([m for m in self.linear_layer if isinstance(m, nn.Linear)])
        return dense_reference_key_map(len(self.output_conv_layer), self.num_units, n_lin)

    def load_reference_state_dict(self, state_dict, prefix=None, strict=True):
        """Load the class-network part of a checkpoint written by the REFERENCE with its dense class network (`class_network.`
        in InstanceSegmentationNetwork).  nn.Conv3d weights [co, ci, a, b, c] become W[(a K + b) K + c, ci, co].  prefix=None:
        detected as in ClassBranch.  -> (missing reference keys, unused checkpoint keys under the prefix)."""
        if prefix is None:
            tail = "input_conv_layer.0.0.0.weight"
            cands = [k[:-len(tail)] for k in state_dict if k.endswith(tail)]
            prefix = next((c for c in cands if c + "linear_layer.1.weight" in state_dict), cands[0] if cands else "")
        converted = {k: (conv3d_to_slab_weight(v) if k.startswith(prefix) and v.dim() == 5 else v) for k, v in state_dict.items()}
        return _load_mapped(self.named_oracle_params(), self.reference_key_map(), converted, prefix,
                            ("input_conv_layer.", "output_conv_layer.", "linear_layer."), strict)


def reshape_reference_key_map(n_same=1, n_linear=2, relu_after_pooling=True):
    """state_dict key of the reference's RESHAPING ClassNetwork -> this package's parameter name
    (`ReshapeClassBranch.named_oracle_params`).  Index 0 of `output_conv_layer` is the parameterless max pool, so the bare
    nn.Conv3d of same-level l sits at l + 1; the input network is an Identity; linear_layer starts with a ReLU only when
    relu_after_pooling (Linear i at 2 i + 1, else at 2 i).  Checked against the key lists of reference
    networks built on the CPU (tests/golden/reshape_class_keys.json)."""
    out = {}
    for t in ("weight", "bias"):
        for l in range(n_same):
            out[f"output_conv_layer.{l + 1}.{t}"] = f"same{l}.{t}"
        for i in range(n_linear):
            out[f"linear_layer.{2 * i + int(bool(relu_after_pooling))}.{t}"] = f"lin{i}.{t}"
    return out


class ReshapeClassBranch(nn.Module):
    """The reference's class network WITHOUT pooling (`simple_class`, scannet_config/run.py:706-710; `cs8_dense8max4_reshape`):
    identity input network, RoiAlign to `cut_shape` (8^3) straight out of the RPN stack's volume at its full width, max pool 2,
    one 3^3 same-convolution per entry of `same_channels` (None keeps the width; a bare nn.Conv3d in the reference: no ReLU before
    or between them), `Reshaper` (channel-major `x.view(R, -1)`, so `linear_layer.1.weight` loads as it is), ReLU Linear ReLU Linear.

    forward(volume_slab [B X Y Z, feature_channels], size, batch, boxes, metadata=None) -> (class_scores [R, num_classes] fp32,
    (bbox_tensor, boxes per sample, size)): DenseClassBranch.forward's contract (`metadata` is accepted for it; the volume
    itself needs no index structure here).  The head computes in fp32: a bf16 volume is widened on entry.  With zero boxes the
    reference raises (`view(0, -1)`); this returns [0, num_classes], as DenseClassBranch does.

    fused=True: RoiAlign and the max pool are ONE pass (functional.RoiAlignPoolFunction: the [R 512, C] samples and their
    gradient are never written -- 126 MB each way at C = 128, R = 480); False: roi.RoiAlign.forward_slab +
    functional.DenseMaxPoolFunction, the same scores bit for bit.  The same-convolutions are SubmanifoldConvolution(3, ., ., 3)
    on the fully active half-size box grids, with DenseClassBranch's BOX_BUCKET bucketing and per-bucket Metadata."""

    def __init__(self, feature_channels, stride, same_channels=(8,), linear_channels=(64,), num_classes=18,
                 cut_shape=(8, 8, 8), relu_after_pooling=True, fused=True):
        super().__init__()
        self.stride = stride
        self.cut_shape = tuple(int(c) for c in cut_shape)
        if len(self.cut_shape) != 3 or any(c % 2 or c < 2 for c in self.cut_shape):
            raise ValueError(f"ReshapeClassBranch: cut_shape {self.cut_shape} must be even per axis (max pool 2)")
        if not len(same_channels):
            raise ValueError("ReshapeClassBranch: at least one same-convolution (same_channels)")
        self.fused, self.relu_after_pooling = bool(fused), bool(relu_after_pooling)
        self.roi_getter = roi.RoiAlign(self.cut_shape, clip_boxes=True, resize_boxes=stride)
        levels, c = [], int(feature_channels)
        for co in same_channels:
            co = c if co is None else int(co)
            levels.append(M.SubmanifoldConvolution(3, c, co, 3, True))
            c = co
        self.output_conv_layer = nn.ModuleList(levels)
        self.half = tuple(v // 2 for v in self.cut_shape)
        c *= self.half[0] * self.half[1] * self.half[2]
        layers = []
        for co in tuple(linear_channels) + (num_classes,):                # (module_factory.py:700-716, start_relu=relu_after_pooling)
            layers += ([nn.ReLU(inplace=bool(layers))] if layers or self.relu_after_pooling else []) + [nn.Linear(c, co)]
            c = co
        self.linear_layer = nn.Sequential(*layers)
        self.num_classes = int(num_classes)
        self._md = {}                         # (size, batch, device) -> fully active Metadata

    __getstate__ = DenseClassBranch.__getstate__
    _metadata = DenseClassBranch._metadata
    bucket = staticmethod(DenseClassBranch.bucket)

    def forward(self, volume_slab, size, batch, boxes, metadata=None):
        from . import functional as F
        from .tensor import SparseConvNetTensor
        size = tuple(int(v) for v in size)
        prev = M.set_feature_storage(torch.float32)
        try:
            if volume_slab.dtype != torch.float32:
                volume_slab = volume_slab.to(torch.float32)
            bbox_tensor, counts, assoc = roi.transform_boxes_interpolation(boxes, size, True, self.stride)
            selection = (bbox_tensor, counts, size)
            r = bbox_tensor.shape[0]
            if r == 0:
                return volume_slab.new_zeros((0, self.num_classes)), selection
            rb = self.bucket(r)
            if self.fused:
                sample = assoc.to(device=volume_slab.device, dtype=torch.int32)
                pooled = F.RoiAlignPoolFunction.apply(volume_slab, bbox_tensor, sample, int(batch), size, self.cut_shape, rb)
            else:
                box_slab, _ = self.roi_getter.forward_slab(volume_slab, size, batch, boxes)
                pooled = F.DenseMaxPoolFunction.apply(box_slab, r, self.cut_shape, rb)
            box_md = self._metadata(self.half, rb, volume_slab.device)
            x = SparseConvNetTensor(pooled, box_md, torch.as_tensor(self.half, dtype=torch.long))
            for conv in self.output_conv_layer:                  # bare convolutions, one after the other
                x = conv(x)
            per = self.half[0] * self.half[1] * self.half[2]
            vectors = F.BoxFlattenFunction.apply(x.features[:r * per], r, self.relu_after_pooling)
        finally:
            M.set_feature_storage(prev)
        return self._linear(vectors), selection

    def _linear(self, x):
        """linear_layer behind the flatten, which has applied its first ReLU already (relu_after_pooling)."""
        from . import functional as F
        for i, m in enumerate(self.linear_layer):
            if isinstance(m, nn.Linear):
                x = F.NetworkInNetworkFunction.apply(x, m.weight.t(), m.bias)
            elif i:                                              # (a ReLU at index 0 ran inside the flatten)
                x = F.ReLUFunction.apply(x)
        return x

    def named_oracle_params(self):
        out = {}
        for l, cv in enumerate(self.output_conv_layer):
            out[f"same{l}.weight"], out[f"same{l}.bias"] = cv.weight, cv.bias
        for i, m in enumerate(m for m in self.linear_layer if isinstance(m, nn.Linear)):
            out[f"lin{i}.weight"], out[f"lin{i}.bias"] = m.weight, m.bias
        return out

    def reference_key_map(self):
        n_lin = len([m for m in self.linear_layer if isinstance(m, nn.Linear)])
        return reshape_reference_key_map(len(self.output_conv_layer), n_lin, self.relu_after_pooling)

    def load_reference_state_dict(self, state_dict, prefix=None, strict=True):
        """Load the class-network part of a checkpoint written by the REFERENCE with its reshaping class network
        (`class_network.` in InstanceSegmentationNetwork).  nn.Conv3d weights [co, ci, a, b, c] become W[(a 3 + b) 3 + c, ci, co];
        the linear weights load as they are (both sides flatten channel-major).  prefix=None: the first key ending in
        'output_conv_layer.1.weight' (a 5-d tensor) with a 'linear_layer.1.weight' sibling.
        -> (missing reference keys, unused checkpoint keys under the prefix)."""
        if prefix is None:
            tail = "output_conv_layer.1.weight"
            cands = [k[:-len(tail)] for k, v in state_dict.items() if k.endswith(tail) and v.dim() == 5]
            prefix = next((c for c in cands if c + "linear_layer.1.weight" in state_dict), cands[0] if cands else "")
        converted = {k: (conv3d_to_slab_weight(v) if k.startswith(prefix) and v.dim() == 5 else v) for k, v in state_dict.items()}
        return _load_mapped(self.named_oracle_params(), self.reference_key_map(), converted, prefix,
                            ("input_conv_layer.", "output_conv_layer.", "linear_layer."), strict)


class SegmentationHead(nn.Module):
    """forward(SparseConvNetTensor of `channels` channels at full resolution) -> fp32 class scores [points, num_classes]
    (bf16-stored features are widened on entry)."""

    def __init__(self, channels, num_classes=20):
        super().__init__()
        self.channel_changer = M.SubmanifoldConvolution(3, channels, num_classes, 1, True)
        self.output_layer = OutputLayer(3)
        self.num_classes = int(num_classes)

    def forward(self, x):
        if x.features.dtype != torch.float32:                    # bf16 storage: 20 columns have no bf16 slab form; widen the input
            x = M.CastFeatures(torch.float32)(x)
        return self.output_layer(self.channel_changer(x))

    def named_oracle_params(self):
        return {"weight": self.channel_changer.weight, "bias": self.channel_changer.bias}

    @staticmethod
    def reference_key_map():
        return {"channel_changer.weight": "weight", "channel_changer.bias": "bias"}

    def load_reference_state_dict(self, state_dict, prefix=None, strict=True):
        """The reference's SegmentationNetwork (`segmentation_network.` in InstanceSegmentationNetwork)."""
        if prefix is None:
            tail = "channel_changer.weight"
            # (the U-Net decoder's SkipConnectionReuniters have channel_changers too: under `module_list`)
            prefix = next((k[:-len(tail)] for k in state_dict if k.endswith(tail) and "module_list" not in k), "")
        return _load_mapped(self.named_oracle_params(), self.reference_key_map(), state_dict, prefix,
                            ("channel_changer.",), strict)
