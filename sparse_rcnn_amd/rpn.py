"""RPN boundary of the detection + mask step (BASELINE configs[2] "Backbone + RPN + sparse ROI-crop mask
head"): the proposals of a step come out of the SAME forward that feeds the mask head.

    encoder level (sparse, stride 8)  --scn.SparseToDense-->  dense [B, C, X/8, Y/8, Z/8]
        --dilation stack (Conv3d 3^3 + ReLU; engine "tiles", the default: this library's tile kernels on a fully active grid;
          engine "miopen": torch.nn.functional.conv3d -- SURVEY §2 row 8 leaves the dense RPN to PyTorch)-->
        --1x1x1 head--> per anchor 6 box deltas + 1 score          (anchor_network.py:73-124 `AnchorNetworkConv`)
          or, MultiLevelRpn(extra_stride_levels=...), the reference's committed choice: per level one transposed convolution
          (kernel = stride) per group of anchors, on a grid finer than the level's (anchor_network.py:127-219
          `AnchorNetworkUpsample`): one row GEMM per level + the scatter of scn_anchor_up.hip
        --anchors that leave the scene dropped: deltas / scores / anchors compacted (anchor.py:103-113, :177-197)-->
        --RoiSelector: detach, sigmoid, top-k (scn_topk_boxes), decode + clip the selected anchors, greedy NMS (scn_nms_bits), keep `post`-->
        list of fp32 boxes [n_i, 2, 3] per sample                    (proposal_selector.py:23-89; bbox.py:139-165,367-398)

What this package contributes to it: SparseToDense (A13, scn_elem.hip), the one-launch NMS (proposals.py) and the consumer
of the boxes (roi.SparseRoiCut).  The dense layers are plain torch modules with the reference's structure
(module_factory.py:581-611 `get_dilation_network`: `num_dilations` x [same convolution + ReLU] behind a SparseToDense;
`get_same_convolution` :396-414: kernel 3, dilation 1, padding 1) -- nn.Conv3d parameters with the reference's names / shapes.

Two engines evaluate those layers (same parameters, same mathematics):
  "miopen"  torch.nn.functional.conv3d on the NCDHW volume.  On this stack MIOpen takes its GEMM fallback solvers for the 3-D
            backward passes (im2col, 450 MB of workspace): 2.4 ms forward but 43 ms forward + backward in fp32, 22 ms under
            bf16 autocast, for a 64 x 64 x 32 volume -- five times the whole sparse step (profiles/r5_dense_rpn_probe.txt).
  "tiles"   (default) a dense same-convolution IS a submanifold convolution on a grid whose every site is active: the volume
            is kept channels-last as the feature slab [B X Y Z, C] of a fully active Metadata (built once per volume shape and
            kept), and the 3^3 layers run on this package's tile kernels (k_conv_ts / k_conv_tb, k_wgrad_*), the 1x1 head on
            the row GEMM.  W_scn[(a*3+b)*3+c, ci, co] = W_torch[co, ci, a, b, c] (SURVEY Appendix B dense identity).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import modules as M
from .proposals import ProposalSelector

class _DilateGather(torch.autograd.Function):
    """h[cell] = bias + sum_o P[map[cell + d_o]][o]  (scn_dilate_gather_fwd / _bwd): the scatter half of a dense 3^3
    same-convolution whose input volume is non-zero on the active rows only; P = X @ [W[0] | ... | W[26]] is one row GEMM."""

    @staticmethod
    def forward(ctx, P, bias, cmap, cell_of_row, batch, size):
        from . import functional as F
        P = F._feat(P)
        hb = P.dtype == torch.bfloat16
        n, c = P.shape[0], P.shape[1] // 27
        cells = batch * size[0] * size[1] * size[2]
        out = torch.empty((cells, c), dtype=P.dtype, device=P.device)
        hs = L.host_i64(3)
        hs[0], hs[1], hs[2] = size
        b = None if bias is None else F._f32(bias)
        L.check(L.lib().scn_dilate_gather_fwd(L.ptr(P), L.ptr(cmap), batch, hs, c, 1 if hb else 0, L.ptr(b), L.ptr(out), L.stream()))
        ctx.save_for_backward(cell_of_row)
        ctx.meta = (n, c, tuple(size), hb, bias is not None)
        return out

    @staticmethod
    def backward(ctx, dOut):
        from . import functional as F
        (cell_of_row,) = ctx.saved_tensors
        n, c, size, hb, has_bias = ctx.meta
        dOut = dOut.to(torch.bfloat16).contiguous() if hb else F._f32(dOut)
        dP = torch.empty((n, 27 * c), dtype=dOut.dtype, device=dOut.device)
        hs = L.host_i64(3)
        hs[0], hs[1], hs[2] = size
        L.check(L.lib().scn_dilate_gather_bwd(L.ptr(dOut), L.ptr(cell_of_row), n, hs, c, 1 if hb else 0, L.ptr(dP), L.stream()))
        db = F.colsum(dOut) if has_bias else None
        return dP, db, None, None, None, None


# the reference's anchor table (scannet_config/network.py:7-23, metres) at its input voxel size with the up-convoluted anchor
# network (run.py:361: 0.0375 m): the three small anchors on the first anchor level, the eleven large ones on the second
REF_RAW_ANCHORS_M = ((0.3752, 0.3752, 0.4221), (0.6566, 0.6566, 0.5159), (0.6566, 0.6566, 0.9380), (0.4221, 0.4221, 1.6415),
                     (0.1876, 1.3132, 1.0318), (0.3283, 0.9849, 1.8291), (0.7035, 1.5008, 0.8442), (1.3132, 0.1876, 1.0318),
                     (0.9849, 0.3283, 1.7822), (1.5008, 0.7035, 0.8442), (0.8442, 2.1574, 0.3752), (2.1574, 0.8442, 0.3752),
                     (2.4857, 1.1256, 1.0318), (1.1256, 2.4857, 1.0318))
REF_VOXEL_M = 0.0375
REF_ANCHOR_LEVELS_VOXELS = tuple(tuple(tuple(v / REF_VOXEL_M for v in a) for a in lv)
                                 for lv in (REF_RAW_ANCHORS_M[:3], REF_RAW_ANCHORS_M[3:]))


def strides_anchors(anchors, basis, min=1, max=None, order=None):
    """`get_strides_anchors` (scannet_config/network.py:24-33): the extra stride of an anchor is round(basis / its edges),
    clipped to [min, max]; anchors with the same stride form a group.  anchors [A, 3] -> (the groups' anchors, a list of
    [A_g, 3] arrays in the order of the sorted unique strides, strides int64 [G, 3], order: the position of every grouped anchor
    in `anchors`).  The strides, the groups and their members are a function of the anchors.  The order of the members INSIDE
    a group is not: the reference takes numpy's default argsort of the group index, which is not a stable sort (numpy's
    vectorised sort puts the two anchors of the reference's group (1, 1, 1) of level 1 in descending order and leaves the two
    of (1, 1, 3) ascending), and so does this function unless `order` fixes it."""
    anchors = np.asarray(anchors, dtype=np.float64)
    inverse_raw = (basis / anchors).round().astype(np.int64).clip(min=min, max=max)
    strides, inverse, counts = np.unique(inverse_raw, return_inverse=True, return_counts=True, axis=0)
    inverse = inverse.reshape(-1)
    if order is None:
        order = np.argsort(inverse)
    else:
        order = np.asarray(order, dtype=np.int64)
        if sorted(order.tolist()) != list(range(len(anchors))) or (np.diff(inverse[order]) < 0).any():
            raise ValueError("strides_anchors: `order` does not list the anchors group by group")
    return np.split(anchors[order], np.cumsum(counts[:-1]), axis=0), strides, order


# the member order of the reference's groups as its configuration produces it (what a checkpoint's `A_g * 7` output channels
# follow): recorded from a run of scannet_config/network.py, fixed here because numpy's default sort does not promise it
REF_UPSAMPLE_ANCHOR_ORDER = ((1, 2, 0), (10, 9, 7, 8, 6, 5, 4, 3, 0, 2, 1))


def _ref_upsample_tables():
    strides, groups = [], []
    for lv, basis, order in zip((REF_RAW_ANCHORS_M[:3], REF_RAW_ANCHORS_M[3:]), (0.6, 1.2), REF_UPSAMPLE_ANCHOR_ORDER):  # network.py:36-41
        g, s, _ = strides_anchors(lv, basis, order=order)
        strides.append(tuple(tuple(int(v) for v in row) for row in s))
        groups.append(tuple(tuple(tuple(float(v) for v in a) for a in (np.asarray(grp) / REF_VOXEL_M)) for grp in g))
    return tuple(strides), tuple(groups)


# the reference's up-sampling heads (run.py:532-537, 830-833): per anchor level the extra strides of its groups and the groups'
# anchors in voxels -- level 0: (1,1,1) x 2 anchors, (2,2,1) x 1; level 1: nine groups, 11 anchors
REF_EXTRA_STRIDE_LEVELS, REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS = _ref_upsample_tables()

# anchor edge lengths in voxels at the one anchor level (stride 8); the synthetic boxes of cfg 3 have edges 8-96
DEFAULT_ANCHORS = ((12.0, 12.0, 12.0), (24.0, 24.0, 24.0), (48.0, 48.0, 32.0), (96.0, 96.0, 48.0))


def fully_active_metadata(size, batch, device):
    """Metadata of the grid `size` with EVERY site of every sample active, rows in (b, x, y, z) order -- row r is cell r of the
    channels-last volume [B, X, Y, Z, C].  Depends on the shape only (DenseRpn.dense_metadata and classhead.DenseClassBranch
    keep what they built)."""
    from .metadata import Metadata
    X, Y, Z = (int(v) for v in size)
    g = torch.stack(torch.meshgrid(torch.arange(batch), torch.arange(X), torch.arange(Y), torch.arange(Z), indexing="ij"),
                    -1).reshape(-1, 4)
    coords = g[:, [1, 2, 3, 0]].contiguous().to(torch.int64)          # (x, y, z, batch), batch-major rows
    return Metadata(3).build_native((X, Y, Z), coords.to(device), batch, 4, 1, 3)


class DenseRpn(nn.Module):
    """`DenseRpn(channels, stride)`: SparseToDense -> dilation stack -> AnchorNetworkConv-style head.
    forward(level_tensor) -> (rpn_bbox [B, N, 2, 3] = (position delta, log-size delta), rpn_score [B, N] raw,
    anchors [N, 2, 3] = (centre, size)), N = X' Y' Z' x A, spatial-major / anchor-minor."""

    ENGINE = "tiles"            # class-wide default: "tiles" | "miopen"
    # "tiles": the FIRST layer of the stack sees a volume that is non-zero on the active rows only (2.3 % of the cells at the
    # stride-8 level of the cfg-2 scene): it runs as ONE row GEMM over the active rows, P = X @ [W[0] | ... | W[26]], + a
    # dilation gather (scn_dilate_gather_*) -- 1.3 GFLOP instead of the volume's 58; False: on the tile kernels like the rest
    SPARSE_FIRST = True

    def __init__(self, channels, stride=8, width=32, num_dilations=2, anchors=DEFAULT_ANCHORS, autocast_bf16=False, engine=None,
                 keep_inside=True, allowed_border=0, keep_volume=False, with_head=True):
        """with_head=False (MultiLevelRpn with up-sampling heads): no 1x1 head is constructed and `forward` hands over the
        stack's output slab, (fp32 slab [B X Y Z, width], size, batch, pinned cell flags); engine "tiles" only.  On a
        bf16-stored level tensor the stack stays bf16-stored through its last ReLU (functional.ReLUFunction on the bf16 slab) and the slab
        handed over is that result widened: the heads' row GEMM, P, the scatter and rpn_bbox / rpn_score are fp32.
        keep_volume (off: nothing changes): keep the stack's output volume -- after its last ReLU, before the head -- of the
        last forward as `self.volume` = (fp32 slab [B X Y Z, width], size, batch, its fully active Metadata): what the
        reference's dense class branch reads (`class_output_anchor`, model.py:435-437).  Engine "tiles" only.  The same
        volume in the stack's stored dtype is `self.volume_stored`: the same tuple with a bf16 slab under autocast_bf16 --
        widening it gives `volume` bit for bit -- and `volume` itself in fp32: what a bf16-stored class branch reads.
        keep_inside: return only the anchors that lie inside the scene (+ allowed_border), as the reference's
        `rpn_bbox_score_splitter` does (anchor.py:103-113,177-197; `allowed_border=0`, scannet_config/run.py:841) -- deltas,
        scores and anchors compacted in anchor order.  The reference's own shape is width 128 / 256 and num_dilations 5
        (run.py:525-536,609): the defaults here are the light stand-in of `--workload cfg3-rpn` (trainstep.py)."""
        super().__init__()
        self.engine = engine
        self.keep_inside, self.allowed_border = bool(keep_inside), float(allowed_border)
        self.keep_volume, self.volume = bool(keep_volume), None
        self._stored = None                   # keep_volume: the stack's stored dtype, then `volume_stored`'s tuple once asked for
        self.channels, self.stride, self.width = int(channels), int(stride), int(width)
        self.to_dense = M.SparseToDense(3, self.channels)
        layers, cin = [], self.channels
        for d in range(num_dilations):                       # get_dilation_network: [same convolution (3^3, dilation 1) + ReLU] x n
            layers += [nn.Conv3d(cin, self.width, 3, padding=1), nn.ReLU(inplace=True)]
            cin = self.width
        self.stack = nn.Sequential(*layers)
        self.register_buffer("anchor_sizes", torch.tensor(anchors, dtype=torch.float32))
        self.n_anchors = len(anchors)
        # anchor_network.py:88-92: num_anchors x (2 x num_dims + 1)
        self.head = nn.Conv3d(cin, self.n_anchors * 7, 1) if with_head else None
        self.autocast_bf16 = bool(autocast_bf16)
        self._anchor_cache = {}
        self._dense_md = {}
        self._flag_host = {}

    def __getstate__(self):
        d = self.__dict__.copy()                 # (the fully active Metadata objects: device index structures, rebuilt on use)
        d["_dense_md"], d["_anchor_cache"], d["_flag_host"] = {}, {}, {}
        d["volume"] = d["_stored"] = None
        return d

    @property
    def volume_stored(self):
        """`volume` with the slab in the dtype the stack stored it in (see __init__).  Behind a 1x1 head the stack's last,
        stand-alone ReLU runs on the widened slab (`_forward_tiles`), so the stored form is `volume` narrowed back on first
        use: exact, every value of it is a bf16 value, and ReLU commutes with the exact widening; a forward that never asks
        launches nothing for it.  With up-sampling heads (with_head=False) that ReLU runs on the bf16 slab itself
        (scn_relu_fwd_bf16) and the stored form is its output tensor: no cast, connected to autograd."""
        if self._stored is None or self.volume is None:
            return None
        if not isinstance(self._stored, tuple):
            x, size, B, dmd = self.volume
            self._stored = (x if x.dtype == self._stored else x.to(self._stored), size, B, dmd)
        return self._stored

    def anchors_for(self, shape, device):
        key = (tuple(shape), str(device))
        a = self._anchor_cache.get(key)
        if a is None:
            g = torch.stack(torch.meshgrid(*[(torch.arange(int(s), dtype=torch.float32) + 0.5) * self.stride for s in shape],
                                           indexing="ij"), -1).reshape(-1, 1, 3)                   # cell centres, voxels
            sz = self.anchor_sizes.detach().cpu().reshape(1, -1, 3)
            a = torch.stack([g.expand(-1, sz.shape[1], -1), sz.expand(g.shape[0], -1, -1)], 2).reshape(-1, 2, 3)
            a = self._anchor_cache[key] = a.to(device)
        return a

    def inside_for(self, shape, device):
        """-> (int64 indices of the anchors of `anchors_for(shape)` that lie inside the scene, those anchors); cached per shape."""
        key = ("inside", tuple(shape), str(device))
        got = self._anchor_cache.get(key)
        if got is None:
            a = self.anchors_for(shape, device)
            scene = torch.tensor([int(v) * self.stride for v in shape], dtype=torch.float32, device=a.device)
            idx = inside_indicator(a, scene, self.allowed_border).nonzero().squeeze(1)
            got = self._anchor_cache[key] = (idx, a[idx])
        return got

    def target_calculator(self, shape, device=None):
        """The reference's `rpn_target_calculator` (anchor.py:148-165 get_bbox_targets) over exactly the anchors `forward` returns
        for a level of spatial size `shape`: calculator(list of [n_i, 2, 3] boxes) -> (max_overlaps, argmax, bbox_targets)
        (loss.RpnTargetCalculator, scn_rpn_targets)."""
        from .loss import RpnTargetCalculator
        device = device if device is not None else self.head.weight.device
        anchors = self.inside_for(shape, device)[1] if self.keep_inside else self.anchors_for(shape, device)
        return RpnTargetCalculator(anchors)

    def _finish(self, raw, shape):
        """raw [B, N, 7] in anchor order -> (rpn_bbox, rpn_score, anchors), inside-the-scene anchors only when asked."""
        if self.keep_inside:
            idx, anchors = self.inside_for(shape, raw.device)
            raw = raw.index_select(1, idx)
        else:
            anchors = self.anchors_for(shape, raw.device)
        return raw[..., :6].reshape(raw.shape[0], -1, 2, 3), raw[..., 6], anchors

    # ---- "tiles": the dense volume as the slab of a fully active grid ------------------------------------------------------
    def dense_metadata(self, size, batch, device):
        """Metadata of the grid `size` with EVERY site of every sample active, rows in (b, x, y, z) order -- row r is cell
        r of the channels-last volume [B, X, Y, Z, C].  Depends on the shape only: built once, kept."""
        key = (tuple(size), int(batch), str(device))
        md = self._dense_md.get(key)
        if md is None:
            md = self._dense_md[key] = fully_active_metadata(size, batch, device)
        return md

    def _forward_tiles(self, level_tensor):
        from . import functional as F
        feats = level_tensor.features
        md = level_tensor.metadata
        size = tuple(int(v) for v in level_tensor.spatial_size)
        B = md.n_samples
        # cell of every active row, ((b X + x) Y + y) Z + z, and the inverse map (-1 on empty cells): scn_cell_map, one launch
        n_cells = B * size[0] * size[1] * size[2]
        n_rows = feats.shape[0]
        ridx = torch.empty(n_rows, dtype=torch.int64, device=feats.device)
        cmap = torch.empty(n_cells, dtype=torch.int32, device=feats.device)
        flag = torch.empty(1, dtype=torch.int32, device=feats.device)      # (rows outside the volume: none by construction)
        hs = L.host_i64(3)
        hs[0], hs[1], hs[2] = size
        L.check(L.lib().scn_cell_map(L.ptr(md.grid(size).coords), n_rows, B, hs, L.ptr(ridx), L.ptr(cmap), L.ptr(flag), L.stream()))
        dmd = self.dense_metadata(size, B, feats.device)
        ssz = torch.as_tensor(size, dtype=torch.long)
        layers = list(self.stack)
        if self.SPARSE_FIRST and isinstance(layers[0], nn.Conv3d) and layers[0].in_channels % 8 == 0 and layers[0].out_channels % 8 == 0:
            # SparseToDense + the first same-convolution without ever building the (mostly zero) input volume
            conv = layers.pop(0)
            Wall = conv.weight.permute(1, 2, 3, 4, 0).reshape(conv.in_channels, 27 * conv.out_channels)     # [Cin][o][Cout]
            P = F.NetworkInNetworkFunction.apply(feats, Wall, None)
            x = _DilateGather.apply(P, conv.bias, cmap, ridx, B, size)
        else:
            x = feats.new_zeros((B * size[0] * size[1] * size[2], feats.shape[1])).index_copy(0, ridx, feats)   # SparseToDense, channels-last
        relu_in = False
        for layer in layers:
            if isinstance(layer, nn.ReLU):
                relu_in = True                                                  # fused into the next layer's gather
                continue
            W = layer.weight.permute(2, 3, 4, 1, 0).reshape(27, layer.in_channels, layer.out_channels)
            x = M._conv_input(x, layer.in_channels, layer.out_channels, True)
            x = F.SubmanifoldConvolutionFunction.apply(x, W, layer.bias, dmd, ssz, 3, relu_in, None)
            relu_in = False
        stored = x.dtype
        if self.head is None and relu_in and stored == torch.bfloat16:
            # up-sampling heads behind a bf16-stored stack: the pending ReLU runs on the stored slab (scn_relu_fwd_bf16), and its
            # result r IS the stored volume; the heads' fp32 slab is r widened -- relu(widen(x)) bit for bit
            r = F.ReLUFunction.apply(x)
            x = r.float()
            if self.keep_volume:
                self.volume = (x, size, B, dmd)
                self._stored = (r, size, B, dmd)
            return x, size, B, self._flags_to_host(flag)
        x = x.float()
        if relu_in:
            x = F.ReLUFunction.apply(x)
        if self.keep_volume:
            self.volume = (x, size, B, dmd)
            self._stored = stored
        if self.head is None:
            return x, size, B, self._flags_to_host(flag)
        Wh = self.head.weight.reshape(self.head.out_channels, self.head.in_channels).t()
        raw = F.NetworkInNetworkFunction.apply(x, Wh, self.head.bias)           # [B X Y Z, A * 7]: spatial-major, anchor-minor
        out = self._finish(raw.view(B, -1, 7), size)
        # scn_cell_map's count of rows outside the volume (a level tensor whose spatial_size / batch disagrees with its
        # coordinates): copied to pinned memory behind the launch, carried on rpn_score, read by RoiSelector.finish after the
        # host wait it makes anyway
        out[1].cell_flags = [self._flags_to_host(flag)]
        return out

    def _flags_to_host(self, flag):
        fh = self._flag_host.get(str(flag.device))
        if fh is None:
            fh = self._flag_host[str(flag.device)] = torch.zeros(1, dtype=torch.int32).pin_memory()
        fh.copy_(flag, non_blocking=True)
        return fh

    def forward(self, level_tensor):
        if (self.engine or self.ENGINE) == "tiles" and level_tensor.features.is_cuda:
            return self._forward_tiles(level_tensor)
        if self.head is None:
            raise L.ScnError("DenseRpn(with_head=False) hands over the channels-last slab of engine 'tiles' on the MI355X "
                             "(no CPU fallback)")
        if self.keep_volume:
            raise L.ScnError("DenseRpn(keep_volume=True) keeps the channels-last slab of engine 'tiles'; engine 'miopen' has none")
        dense = self.to_dense(level_tensor)                  # [B, C, X', Y', Z'] (bf16 when the slab is bf16-stored)
        if self.autocast_bf16:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                raw = self.head(self.stack(dense))
            raw = raw.float()
        else:
            raw = self.head(self.stack(dense.float()))
        B = raw.shape[0]
        shape = raw.shape[2:]
        raw = raw.view(B, self.n_anchors, 7, -1).permute(0, 3, 1, 2).reshape(B, -1, 7)
        return self._finish(raw, shape)


def inside_indicator(anchors, scene_shape, allowed_border=0.0):
    """AnchorDescriptionMultiLevel.inside_indicator (ndsis/modules/anchor.py:103-113): anchors [N, 2, 3] = (centre, size),
    True where start >= -border and end <= scene_shape + border on every axis (calc_start_end, utils/bbox.py:267-287)."""
    half = anchors[..., 1, :] / 2
    start, end = anchors[..., 0, :] - half, anchors[..., 0, :] + half
    scene_shape = torch.as_tensor(scene_shape, dtype=anchors.dtype, device=anchors.device)
    return torch.all(start >= -allowed_border, dim=-1) & torch.all(end <= scene_shape + allowed_border, dim=-1)


def decode_boxes(anchors, deltas, scene_shape=None):
    """bbox_transform_inv (ndsis/utils/bbox.py:139-165,267-287,367-398): anchors (centre, size), deltas (position, log size)
    -> boxes (start, stop).  fp32, same operation order as the reference.  scene_shape: clip the boxes to [0, scene_shape]
    as `AnchorDescriptionMultiLevel.forward` does (anchor.py:218-227, `clip_boxes` utils/bbox.py:16-34)."""
    pos = deltas[..., 0, :] * anchors[..., 1, :] + anchors[..., 0, :]
    size = torch.exp(deltas[..., 1, :]) * anchors[..., 1, :]
    half = size / 2
    boxes = torch.stack((pos - half, pos + half), dim=-2)
    if scene_shape is not None:
        boxes = torch.min(boxes, torch.as_tensor(scene_shape, dtype=boxes.dtype, device=boxes.device)).clamp(min=0)
    return boxes


class _UpPlan:
    """What AnchorNetworkUpsample keeps per (scene shape, level sizes, device): a function of those alone."""
    __slots__ = ("n_all", "n_inside", "dest", "levels", "anchors", "inside_cpu")


class _Operation(nn.Module):
    """Name holder: the reference wraps its heads as ConcatOutputListList(ZipApply(ModuleMap(...))), which spells their
    parameters `rpn_net_levels.operation.{level}.{group}.weight` / `.bias` (custom_container.py:24-26,87-99)."""

    def __init__(self, level_groups):
        super().__init__()
        self.operation = nn.ModuleList(nn.ModuleList(g) for g in level_groups)


class AnchorNetworkUpsample(nn.Module):
    """The reference's up-sampling RPN heads (ndsis/modules/anchor_network.py:127-219): per anchor level one
    `ConvTranspose3d(C, A_g * 7, kernel = stride = extra_stride_g)` per group g of anchors that share an extra stride, so that a
    group's anchors sit on the level's grid refined by that stride (combined stride conv_stride / extra_stride, fractional).
    raw_anchor_levels: per level the groups' anchors [A_g, 3] in voxels; conv_stride_levels: per level the stride of its
    volume (a number or one per axis); channels_levels: per level C; extra_stride_levels: per level [G, 3] integers.
    Parameters have the reference's shapes ([C, A_g * 7, s0, s1, s2], [A_g * 7]), names
    (`rpn_net_levels.operation.{l}.{g}.*`) and initialisation (nn.ConvTranspose3d's, in the reference's construction order).

    A transposed convolution with kernel = stride has no overlap between taps: level l is ONE row GEMM P = X @ Wm + bias_cols
    on the level's channels-last slab (functional.NetworkInNetworkFunction; Wm [C, Ncol], column col0_g + ((a s1 + b) s2 + c)
    (A_g 7) + co = W_g[ci, co, a, b, c], packed per call with permute / reshape / cat so that autograd carries the gradients
    back to the ConvTranspose3d-shaped parameters) and one scatter into the outputs (functional.AnchorUpFunction,
    scn_anchor_up.hip).

    forward([(slab [B X Y Z, C], size (X, Y, Z), batch)] per level, scene_shape) -> (rpn_bbox [B, N, 2, 3], rpn_score [B, N],
    anchors [N, 2, 3] = (centre, size)) over the anchors inside the scene (+ allowed_border), in the reference's order: groups
    in level order then group order, fine cells row-major with z fastest, the anchor index minor (anchor.py:82-113,171-192)."""

    def __init__(self, raw_anchor_levels, conv_stride_levels, channels_levels, allowed_border=0, *, extra_stride_levels):
        super().__init__()
        if not (len(raw_anchor_levels) == len(conv_stride_levels) == len(channels_levels) == len(extra_stride_levels)):
            raise ValueError("AnchorNetworkUpsample: one entry per level in every argument")
        heads, self._groups = [], []
        for anchors_l, stride_l, c, extra_l in zip(raw_anchor_levels, conv_stride_levels, channels_levels, extra_stride_levels):
            extra_l = np.asarray(extra_l, dtype=np.int64).reshape(-1, 3)
            if len(anchors_l) != len(extra_l) or not 1 <= len(extra_l) <= L.ANCHOR_UP_MAX_GROUPS:
                raise ValueError(f"AnchorNetworkUpsample: {len(anchors_l)} anchor groups, {len(extra_l)} extra strides "
                                 f"(1 .. {L.ANCHOR_UP_MAX_GROUPS} groups per level, one stride each)")
            conv = np.broadcast_to(np.asarray(stride_l), (3,))
            combined = conv / extra_l                                   # float64, as create_level_upsampler divides
            groups = []
            for g, (a, e) in enumerate(zip(anchors_l, extra_l)):
                a = torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=torch.float32).reshape(-1, 3)
                e = tuple(int(v) for v in e)
                if a.shape[0] < 1 or min(e) < 1:
                    raise ValueError("AnchorNetworkUpsample: every group needs an anchor and extra strides >= 1")
                groups.append(dict(extra=e, n_anchors=a.shape[0], raw=a,
                                   stride=torch.as_tensor(combined[g], dtype=torch.float32)))   # AnchorStorage's cast
            self._groups.append(groups)
            heads.append([nn.ConvTranspose3d(int(c), gr["n_anchors"] * 7, gr["extra"], gr["extra"]) for gr in groups])
        self.rpn_net_levels = _Operation(heads)
        self.conv_strides = [tuple(int(v) for v in np.broadcast_to(np.asarray(s), (3,))) for s in conv_stride_levels]
        self.channels_levels = tuple(int(c) for c in channels_levels)
        self.allowed_border = allowed_border
        self._cache = {}

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_cache"] = {}
        return d

    def heads(self):
        """The ConvTranspose3d modules, level-major."""
        return [h for lv in self.rpn_net_levels.operation for h in lv]

    @property
    def ncol_levels(self):
        return tuple(sum(g["extra"][0] * g["extra"][1] * g["extra"][2] * g["n_anchors"] * 7 for g in lv) for lv in self._groups)

    def all_anchors(self, sizes):
        """Every anchor of levels of spatial `sizes`, in all-anchor order, fp32 [N_all, 2, 3] on the host
        (AnchorDescriptionMultiLevel._get_pixelwise_anchors, anchor.py:127-146: centres (arange + 0.5) * stride in fp32)."""
        out = []
        for groups, size in zip(self._groups, sizes):
            for g in groups:
                ranges = [(torch.arange(int(n) * e, dtype=torch.float32) + 0.5) * st
                          for n, e, st in zip(size, g["extra"], g["stride"])]
                shifts = torch.cartesian_prod(*ranges).unsqueeze(-2)
                out.append(torch.stack(torch.broadcast_tensors(shifts, g["raw"]), dim=-2).reshape(-1, 2, 3))
        return torch.cat(out, 0)

    def plan(self, scene_shape, sizes, device):
        sizes = tuple(tuple(int(v) for v in s) for s in sizes)
        key = (tuple(float(v) for v in scene_shape), sizes, str(device))
        pl = self._cache.get(key)
        if pl is None:
            anchors = self.all_anchors(sizes)
            inside = inside_indicator(anchors, torch.tensor(key[0], dtype=torch.float32), self.allowed_border)
            dest = torch.where(inside, torch.cumsum(inside, 0) - 1, torch.full((), -1, dtype=torch.int64)).to(torch.int32)
            pl = _UpPlan()
            pl.n_all, pl.n_inside = int(anchors.shape[0]), int(inside.sum())
            pl.inside_cpu = inside
            pl.anchors = anchors[inside].to(device)
            pl.dest = dest.to(device)
            pl.levels, first = [], 0
            for groups, size, ncol in zip(self._groups, sizes, self.ncol_levels):
                table, col = L.host_i64(6 * len(groups)), 0
                for i, g in enumerate(groups):
                    e, a = g["extra"], g["n_anchors"]
                    table[6 * i:6 * i + 6] = [e[0], e[1], e[2], a, col, first]
                    col += e[0] * e[1] * e[2] * a * 7
                    first += size[0] * size[1] * size[2] * e[0] * e[1] * e[2] * a
                pl.levels.append((size, ncol, table, len(groups)))
            self._cache[key] = pl
        return pl

    def packed(self, level):
        """(Wm [C, Ncol], bias_cols [Ncol]) of a level from its groups' parameters."""
        ws, bs = [], []
        for h in self.rpn_net_levels.operation[level]:
            taps = h.weight.shape[2] * h.weight.shape[3] * h.weight.shape[4]
            ws.append(h.weight.permute(0, 2, 3, 4, 1).reshape(h.weight.shape[0], -1))
            bs.append(h.bias.repeat(taps))
        return torch.cat(ws, 1), torch.cat(bs, 0)

    def level_sizes(self, scene_shape):
        return tuple(tuple(int(v) // s for v, s in zip(scene_shape, st)) for st in self.conv_strides)

    def target_calculator(self, scene_shape, device=None):
        """The reference's `rpn_target_calculator` (anchor.py:148-165) over exactly the inside anchors `forward` returns for a
        scene of `scene_shape` voxels (every level's grid: scene_shape / its stride), as MultiLevelRpn.target_calculator."""
        from .loss import RpnTargetCalculator
        device = device if device is not None else self.heads()[0].weight.device
        scene = tuple(int(v) for v in scene_shape)
        return RpnTargetCalculator(self.plan(scene, self.level_sizes(scene), device).anchors)

    def forward(self, level_slabs, scene_shape):
        from . import functional as F
        if len(level_slabs) != len(self._groups):
            raise ValueError(f"AnchorNetworkUpsample: {len(self._groups)} levels, {len(level_slabs)} slabs")
        if not all(s[0].is_cuda for s in level_slabs):
            raise L.ScnError("AnchorNetworkUpsample: the level slabs must live on the MI355X (no CPU fallback)")
        batch = int(level_slabs[0][2])
        pl = self.plan(scene_shape, [s[1] for s in level_slabs], level_slabs[0][0].device)
        Ps = []
        for l, (slab, size, b) in enumerate(level_slabs):
            if int(b) != batch:
                raise ValueError("AnchorNetworkUpsample: the levels disagree about the batch size")
            Wm, bias_cols = self.packed(l)
            Ps.append(F.NetworkInNetworkFunction.apply(slab, Wm, bias_cols))
        rpn_bbox, rpn_score = F.AnchorUpFunction.apply(pl, batch, *Ps)
        return rpn_bbox, rpn_score, pl.anchors

    def load_reference_state_dict(self, state_dict):
        """Copy a reference checkpoint's head parameters: keys `rpn_net_levels.operation.{l}.{g}.weight` / `.bias`, bare or
        under `bbox_network.` (then every other key of the checkpoint is somebody else's).  The reference's non-learned
        entries (`anchor_storage.conv_stride_levels`, `anchor_storage.raw_anchor_levels.*`, `anchor_storage.descriptions.*`)
        are ignored.  A missing or extra group, or another shape, is a ValueError that names the key; nothing is copied then."""
        prefix = "bbox_network."
        if any(k.startswith(prefix) for k in state_dict):
            state_dict = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        given = {k: v for k, v in state_dict.items() if not k.startswith("anchor_storage.")}
        own = dict(self.named_parameters())
        for k in given:
            if k not in own:
                raise ValueError(f"AnchorNetworkUpsample: the checkpoint's `{k}` has no counterpart (levels / groups: "
                                 f"{[len(g) for g in self._groups]})")
        for k, p in own.items():
            if k not in given:
                raise ValueError(f"AnchorNetworkUpsample: the checkpoint lacks `{k}`")
            if tuple(given[k].shape) != tuple(p.shape):
                raise ValueError(f"AnchorNetworkUpsample: `{k}` is {tuple(given[k].shape)} in the checkpoint, {tuple(p.shape)} here")
        with torch.no_grad():
            for k, p in own.items():
                p.copy_(torch.as_tensor(given[k]).to(p.device, p.dtype))


class MultiLevelRpn(nn.Module):
    """The reference's RPN shape with several anchor levels (scannet_config/run.py:525-536: `upconvoluted_anchornetwork`,
    one dilation network per anchor level, `anchor_output_channels = [128, 256]`, `num_dilations = 5` :609): one DenseRpn per
    level -- SparseToDense of THAT encoder level, its own dilation stack, a 1x1 head for its own anchors -- the levels'
    outputs concatenated in level order and the anchors that leave the scene dropped (`rpn_bbox_score_splitter`,
    anchor.py:177-197).  extra_stride_levels=None: 1x1 heads, every level's anchors on the level's own grid
    (`AnchorNetworkConv`).  extra_stride_levels given (per level [G, 3]): the reference's committed heads, transposed
    convolutions that refine the anchor grid per group of anchors (`AnchorNetworkUpsample` above, as `self.anchor_network`); the
    DenseRpn levels then carry no head and hand over their stack's slab, and a level's anchors are its groups' [A_g, 3] lists.
    levels: [(channels, stride, width, anchors [A, 3] in voxels -- or the groups' anchors)];  forward(level_tensors) ->
    (rpn_bbox [B, N, 2, 3], rpn_score [B, N], anchors [N, 2, 3]) over the inside anchors of all levels."""

    def __init__(self, levels, num_dilations=5, autocast_bf16=False, engine=None, allowed_border=0, keep_volume=False,
                 class_output_index=0, extra_stride_levels=None):
        """keep_volume / class_output_index (off: nothing changes): the level `class_output_index` keeps its stack's output
        volume (DenseRpn(keep_volume=True)), read back as `self.volume`; 0 is the reference's index with segmentation
        (scannet_config/run.py:605-607)."""
        super().__init__()
        self.class_output_index = int(class_output_index)
        up = extra_stride_levels is not None
        self.levels = nn.ModuleList(DenseRpn(c, stride, width, num_dilations, () if up else tuple(map(tuple, a)), autocast_bf16,
                                             engine, keep_inside=False,
                                             keep_volume=bool(keep_volume) and i == self.class_output_index % len(levels),
                                             **(dict(with_head=False) if up else {}))
                                    for i, (c, stride, width, a) in enumerate(levels))
        self.anchor_network = None
        if up:
            self.anchor_network = AnchorNetworkUpsample([a for _, _, _, a in levels], [s for _, s, _, _ in levels],
                                                        [w for _, _, w, _ in levels], allowed_border,
                                                        extra_stride_levels=extra_stride_levels)
        self.allowed_border = float(allowed_border)
        self._cache = {}

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_cache"] = {}
        return d

    @property
    def volume(self):
        return self.levels[self.class_output_index].volume

    @property
    def volume_stored(self):
        return self.levels[self.class_output_index].volume_stored

    def forward(self, level_tensors):
        outs = [rpn(t) for rpn, t in zip(self.levels, level_tensors)]
        scene = tuple(int(v) * self.levels[0].stride for v in level_tensors[0].spatial_size)
        if self.anchor_network is not None:
            rpn_bbox, rpn_score, anchors = self.anchor_network([o[:3] for o in outs], scene)
            rpn_score.cell_flags = [o[3] for o in outs]
            return rpn_bbox, rpn_score, anchors
        return self.combine(outs, scene)

    def _inside(self, level_anchors, scene_shape, device):
        key = (tuple(scene_shape), tuple(a.shape[0] for a in level_anchors), str(device))
        got = self._cache.get(key)
        if got is None:
            anchors = torch.cat(level_anchors, 0)
            idx = inside_indicator(anchors, torch.tensor(scene_shape, dtype=torch.float32), self.allowed_border).nonzero().squeeze(1)
            got = self._cache[key] = (idx, anchors[idx])
        return got

    def target_calculator(self, scene_shape, device=None):
        """The reference's `rpn_target_calculator` (anchor.py:148-165 get_bbox_targets) over exactly the inside anchors
        `forward` returns for a scene of `scene_shape` voxels (every level's grid: scene_shape / its stride)
        (loss.RpnTargetCalculator, scn_rpn_targets)."""
        from .loss import RpnTargetCalculator
        if self.anchor_network is not None:
            return self.anchor_network.target_calculator(scene_shape, device)
        device = device if device is not None else self.levels[0].head.weight.device
        scene = tuple(int(v) for v in scene_shape)
        level_anchors = [l.anchors_for(tuple(v // l.stride for v in scene), device) for l in self.levels]
        return RpnTargetCalculator(self._inside(level_anchors, scene, device)[1])

    def combine(self, outs, scene_shape):
        """Per-level (rpn_bbox, rpn_score, anchors) over ALL anchors of each level -> the reference's concatenation in level
        order with the anchors that leave `scene_shape` dropped (`rpn_bbox_score_splitter`, anchor.py:177-197)."""
        idx, anchors = self._inside([o[2] for o in outs], tuple(scene_shape), outs[0][0].device)
        rpn_bbox = torch.cat([o[0] for o in outs], 1).index_select(1, idx)
        rpn_score = torch.cat([o[1] for o in outs], 1).index_select(1, idx)
        rpn_score.cell_flags = [f for o in outs for f in getattr(o[1], "cell_flags", [])]
        return rpn_bbox, rpn_score, anchors


class RoiSelector(nn.Module):
    """`RoiSelector(num_keep_pre_nms, num_keep_post_nms, thresh_nms, detach=True)` (proposal_selector.py:23-50):
    forward(rpn_bbox, rpn_score, anchors[, scene_shape]) -> (roi_score, roi_bbox, roi_index) lists per sample.  `anchors` is
    either the anchors tensor [N, 2, 3] (decoded with `decode_boxes` AFTER the top-k, clipped to `scene_shape` when given) or --
    the reference's own third argument -- a callable `anchor_description` that maps rpn_bbox to boxes (decoded before the top-k)."""

    def __init__(self, num_keep_pre_nms=1024, num_keep_post_nms=64, thresh_nms=0.5, detach=True):
        super().__init__()
        self.proposal_selector = ProposalSelector(num_keep_pre_nms, num_keep_post_nms, thresh_nms)
        self.detach = detach
        self._scene_cache = {}                   # (scene shape, device) -> device tensor: no host-to-device copy per step

    def forward(self, rpn_bbox, rpn_score, anchors, scene_shape=None):
        return self.finish(self.start(rpn_bbox, rpn_score, anchors, scene_shape))

    def start(self, rpn_bbox, rpn_score, anchors, scene_shape=None):
        """Everything up to and including the NMS launch, nothing awaited (ProposalSelector.start).  scene_shape: the
        proposals are clipped to the scene, as `anchor_description(rpn_bbox)` does in the reference (anchor.py:218-227)."""
        flags = getattr(rpn_score, "cell_flags", [])
        if self.detach:
            rpn_bbox, rpn_score = rpn_bbox.detach(), rpn_score.detach()
        if callable(anchors) and not torch.is_tensor(anchors):
            # the reference's own call: `anchor_description(rpn_bbox)` -- an AnchorDescriptionMultiLevel (anchor.py:218-227) or
            # any callable that turns the deltas into clipped (start, stop) boxes -- decodes every anchor before the selection
            return self.proposal_selector.start(torch.sigmoid(rpn_score), anchors(rpn_bbox)) + (flags,)
        if scene_shape is not None and not torch.is_tensor(scene_shape):
            key = (tuple(float(v) for v in scene_shape), str(rpn_bbox.device))
            t = self._scene_cache.get(key)
            if t is None:
                t = self._scene_cache[key] = torch.tensor(key[0], dtype=torch.float32, device=rpn_bbox.device)
            scene_shape = t
        decode = decode_boxes if scene_shape is None else (lambda a, d: decode_boxes(a, d, scene_shape))
        return self.proposal_selector.start_from_deltas(torch.sigmoid(rpn_score), rpn_bbox, anchors, decode) + (flags,)

    def finish(self, state):
        out = self.proposal_selector.finish(state[:4])          # (waits on the host: the pinned cell flags are complete)
        if any(int(f[0]) != 0 for f in state[4]):
            raise L.ScnError("DenseRpn: rows of a level tensor lie outside its spatial_size / batch (scn_cell_map counted "
                             f"{[int(f[0]) for f in state[4]]}): its Metadata and its coordinates disagree")
        return out


class _TrainValSelector(nn.Module):
    """Training-mode / evaluation-mode pair of selectors (the reference wraps its two RoiSelectors in a `ConditionalStage`,
    custom_container.py:102-116: every call and attribute goes to the member that matches `self.training`)."""

    def __init__(self, train_module, val_module):
        super().__init__()
        self.train_module, self.val_module = train_module, val_module

    def _member(self):
        return self.train_module if self.training else self.val_module

    def forward(self, *a, **kw):
        return self._member()(*a, **kw)

    def start(self, *a, **kw):
        return self._member().start(*a, **kw)

    def finish(self, state):
        return self._member().finish(state)


def get_roi_selector(num_keep_pre_nms=1000, num_keep_post_nms=500, thresh_nms=0.5, val_num_keep_pre_nms=None,
                     val_num_keep_post_nms=None, val_thresh_nms=None):
    """`get_roi_selector` (proposal_selector.py:6-20) with the reference's defaults: one RoiSelector, or -- when evaluation has
    its own numbers (scannet_config/run.py:847-853: 1024 / 256 / 0.5 in training, 1024 / 32 or 256 / 0.3 in evaluation) -- a pair
    that follows `module.training`."""
    sel = RoiSelector(num_keep_pre_nms, num_keep_post_nms, thresh_nms)
    if val_num_keep_pre_nms:
        sel = _TrainValSelector(sel, RoiSelector(val_num_keep_pre_nms, val_num_keep_post_nms, val_thresh_nms))
    return sel
