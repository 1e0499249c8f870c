"""The dense class network written from the specification (1^3 convolution + residual units on the volume, RoiAlign,
max pool 2, [2^3/2 convolution + units] per level, mean over the remaining sites, ReLU Linear ReLU Linear) with the three
hooks a bf16-STORED evaluation needs, and the fp32 emulation of the bf16 RoiAlign entry points the CPU bounds are checked on.

Hooks (identity by default: the reference's own fp32 network):
  q     rounding of every STORED slab.  Placed where oracle/scn_oracle.py's `unet_forward` / `dense_rpn_forward` place
        `storage` for the same layer kinds -- after a 1^3 or a strided convolution, after the FIRST convolution of a residual
        unit, after the unit's sum x + y (the second convolution's result is added before anything is stored) -- and, for the
        two operators of the branch, after RoiAlign and after the max pool (the maximum of stored values: a no-op for bf16).
        The mean, the linear layers and the scores are fp32: no q.
  wq    rounding of the weights of the layers that run on the bf16 tile kernels: the 3^3 and the 2^3/2 convolutions
        (`tile_weights`); the 1^3 convolution is a row GEMM with fp32 weights, the linear layers are fp32.
  relu  torch.relu, or prescribed sign masks (`FrozenMasks`: the masks a device forward recorded, in call order), always
        called on channels-last rows [sites, C] -- the layout of the device's slabs.
The backward of `bf16_round` is straight-through, as oracle.scn_oracle.bf16_storage.
"""
import numpy as np
import torch
import torch.nn.functional as TF

import roialign_restate as R


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def bf16_round(t):
    """Round to nearest-even bf16, widened back to the argument's dtype; straight-through gradient."""
    return _Round.apply(t)


def identity(t):
    return t


class FrozenMasks:
    """relu hook with prescribed sign masks: call k multiplies its argument [rows, C] by mask k.  A mask may have more rows
    (the device pads the box count to a bucket; the real boxes come first) or more columns than the argument."""

    def __init__(self, masks):
        self.masks, self.k = list(masks), 0

    def __call__(self, x):
        m = self.masks[self.k]
        self.k += 1
        if m.shape[0] < x.shape[0] or m.shape[1] < x.shape[1]:
            raise ValueError(f"FrozenMasks: mask {self.k - 1} has shape {tuple(m.shape)}, argument {tuple(x.shape)}")
        return x * m[:x.shape[0], :x.shape[1]].to(x.dtype)


def _rows(fn, h):
    """fn on the channels-last rows of an NCDHW tensor, back to NCDHW."""
    n, c = h.shape[:2]
    rows = fn(h.permute(0, 2, 3, 4, 1).reshape(-1, c))
    return rows.view(n, *h.shape[2:], c).permute(0, 4, 1, 2, 3)


def dense_class_forward(sd, volume_ncxyz, bbox_batch, stride, cut_shape, n_levels=2, num_units=1, q=identity, wq=identity,
                        relu=torch.relu):
    """sd: the reference's state dict (its keys, nn.Conv3d / nn.Linear layouts).  volume_ncxyz [B, C, X, Y, Z] as stored (the
    caller rounds it).  -> (class scores [R, classes], bbox_tensor fp32 [R, 2, 3], counts)."""
    def unit(x, prefix):
        y = q(TF.conv3d(_rows(relu, x), wq(sd[prefix + "inner_block.1.weight"]), sd[prefix + "inner_block.1.bias"], padding=1))
        y = TF.conv3d(_rows(relu, y), wq(sd[prefix + "inner_block.3.weight"]), sd[prefix + "inner_block.3.bias"], padding=1)
        return q(x + y)

    x = q(TF.conv3d(volume_ncxyz, sd["input_conv_layer.0.0.0.weight"], sd["input_conv_layer.0.0.0.bias"]))
    for u in range(num_units):
        x = unit(x, f"input_conv_layer.0.1.{u}.")
    size = x.shape[2:]
    bbox_tensor, counts, sample = R.transform_boxes(bbox_batch, size, stride, True)
    cut = q(R.roialign(x.permute(0, 2, 3, 4, 1), bbox_tensor, sample, cut_shape)).permute(0, 4, 1, 2, 3)
    x = q(TF.max_pool3d(cut, 2))
    for l in range(1, n_levels + 1):
        x = q(TF.conv3d(x, wq(sd[f"output_conv_layer.{l}.0.0.weight"]), sd[f"output_conv_layer.{l}.0.0.bias"], stride=2))
        for u in range(num_units):
            x = unit(x, f"output_conv_layer.{l}.1.{u}.")
    x = x.mean(dim=(2, 3, 4))
    x = TF.linear(relu(x), sd["linear_layer.1.weight"], sd["linear_layer.1.bias"])
    x = TF.linear(relu(x), sd["linear_layer.3.weight"], sd["linear_layer.3.bias"])
    return x, bbox_tensor, counts


# ---- the bf16 RoiAlign entry points, emulated: fp32 arithmetic on bf16 inputs, ONE rounding of the result ---------------------
WIDTHS = (8, 32, 40)                  # one 16-byte lane per row, the workload's width, a partial wave
GEOMETRIES = ("mixed", "small8", "aniso", "whole40")
OUT_REL, OUT_ABS = 2.0 ** -8, 2.1e-6  # |got - ref| <= 2^-8 |ref| + 2.1e-6 max|F|: one bf16 rounding (half an ulp = 2^-9 of a
#                                       value in [2^e, 2^(e+1)), so <= 2^-8 |v| with room for v itself being off) on top of the
#                                       fp32 kernel's own 2e-6 max|F| bar against float64 (tests/test_roialign_cpu.py)
GRAD_BAR = 2.0 ** -8 + 2e-5           # relative L2: one rounding per element plus the fp32 gradient bar


def bf16_case(z, c):
    """The geometry of fixture `z` at width c with seeded, bf16-representable inputs (fp32 arrays):
    -> (volume [B, X, Y, Z, c], boxes [R, 2, 3], sample_of_box int64 [R], dout [R, ex, ey, ez, c])."""
    vol = bf16_round(torch.from_numpy(R.seeded_volume(40 + c, z["_batch"], z["_size"], c)))
    boxes = torch.from_numpy(z["bbox_tensor"])
    sample = torch.tensor([s for s, n in enumerate(z["counts"]) for _ in range(int(n))], dtype=torch.long)
    dout = bf16_round(torch.from_numpy(R.seeded_dout(40 + c, boxes.shape[0], z["_extract"], c)))
    return vol, boxes, sample, dout


_REF = {}


def float64_reference(name, z, c):
    """R.roialign in float64 on the bf16 inputs of `bf16_case` -> (out, d volume), float64; computed once per (case, width)."""
    if (name, c) not in _REF:
        vol, boxes, sample, dout = bf16_case(z, c)
        v = vol.double().requires_grad_()
        out = R.roialign(v, boxes.double(), sample, z["_extract"])
        out.backward(dout.double())
        _REF[(name, c)] = (out.detach(), v.grad)
    return _REF[(name, c)]


def forward_slack(got, ref, absmax):
    """max over elements of |got - ref| - (OUT_REL |ref| + OUT_ABS max|F|): <= 0 passes."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float(((got - ref).abs() - (OUT_REL * ref.abs() + OUT_ABS * absmax)).max())


def rel_l2(got, ref):
    return R.rel_l2(np.asarray(got, np.float64), np.asarray(ref, np.float64))
