"""Helpers of the up-sampling RPN head tests (test_anchor_up_cpu.py, test_gpu_anchor_up.py): the fixtures the reference's
AnchorNetworkUpsample wrote (tests/golden/make_anchor_up_golden.py) and a restatement of the head in torch operators --
packed weights, matmul, then per group view / permute / reshape, a cat over the groups, the inside mask, the split into box
deltas and score.  It shares nothing with the device code but the definition of the column layout."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("all_inside", "mixed", "border")


class Fixture:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, f"anchor_up_{name}.npz"))
        self.z = z
        self.name = name
        self.scene = tuple(int(v) for v in z["scene_shape"])
        self.border = float(z["border"])
        self.batch = int(z["batch"])
        self.conv_strides = [int(v) for v in z["conv_strides"]]
        self.n_levels = int(z["n_levels"])
        self.sizes = [tuple(v // s for v in self.scene) for s in self.conv_strides]
        self.extra = [[tuple(int(v) for v in e) for e in z[f"extra_strides{l}"]] for l in range(self.n_levels)]
        self.anchors = [[z[f"anchors{l}_{k}"] for k in range(int(z[f"n_groups{l}"]))] for l in range(self.n_levels)]
        self.channels = [int(z[f"feat{l}"].shape[1]) for l in range(self.n_levels)]
        self.groups = [[(e, len(a)) for e, a in zip(self.extra[l], self.anchors[l])] for l in range(self.n_levels)]
        self.inside = torch.from_numpy(z["inside_indicator"])

    def t(self, key):
        return torch.from_numpy(self.z[key])

    def slab(self, l):
        """The level's volume [B, C, X, Y, Z] as the channels-last slab [B X Y Z, C]."""
        f = self.t(f"feat{l}")
        return f.permute(0, 2, 3, 4, 1).reshape(-1, f.shape[1]).contiguous()

    def dslab(self, l):
        f = self.t(f"dfeat{l}")
        return f.permute(0, 2, 3, 4, 1).reshape(-1, f.shape[1]).contiguous()

    def module(self):
        """rpn.AnchorNetworkUpsample with the fixture's anchors, strides, border and weights."""
        from sparse_rcnn_amd import rpn as R
        net = R.AnchorNetworkUpsample(self.anchors, self.conv_strides, self.channels, self.border, extra_stride_levels=self.extra)
        with torch.no_grad():
            for l, lv in enumerate(net.rpn_net_levels.operation):
                for k, h in enumerate(lv):
                    h.weight.copy_(self.t(f"w{l}_{k}"))
                    h.bias.copy_(self.t(f"b{l}_{k}"))
        return net


_fixtures = {}


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = Fixture(name)
    return _fixtures[name]


def keys_doc():
    with open(os.path.join(GOLDEN, "anchor_up_keys.json")) as f:
        return json.load(f)


def pack(weights, biases):
    """Per-group ConvTranspose3d parameters ([C, A7, s0, s1, s2], [A7]) -> (Wm [C, Ncol], bias_cols [Ncol]): column
    col0_g + ((a s1 + b) s2 + c) A7 + co = W_g[ci, co, a, b, c]."""
    ws, bs = [], []
    for w, b in zip(weights, biases):
        ws.append(w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1))
        bs.append(b.repeat(w.shape[2] * w.shape[3] * w.shape[4]))
    return torch.cat(ws, 1), torch.cat(bs, 0)


def all_records(P, batch, size, groups):
    """P [B X Y Z, Ncol] -> [B, N_level, 7]: the level's records in all-anchor order (groups in order, fine cells row-major
    over (X s0, Y s1, Z s2) with z fastest, anchor minor)."""
    X, Y, Z = size
    out, col = [], 0
    for (s0, s1, s2), a in groups:
        n = s0 * s1 * s2 * a * 7
        blk = P[:, col:col + n].reshape(batch, X, Y, Z, s0, s1, s2, a, 7)
        out.append(blk.permute(0, 1, 4, 2, 5, 3, 6, 7, 8).reshape(batch, -1, 7))
        col += n
    assert col == P.shape[1]
    return torch.cat(out, 1)


def permute_restated(Ps, batch, sizes, groups_levels, inside):
    """The torch-operator form of functional.AnchorUpFunction: -> (rpn_bbox [B, N_in, 2, 3], rpn_score [B, N_in])."""
    rec = torch.cat([all_records(P, batch, s, g) for P, s, g in zip(Ps, sizes, groups_levels)], 1)
    rec = rec[:, inside.to(rec.device)]
    return rec[..., :6].reshape(batch, -1, 2, 3), rec[..., 6]


def head_restated(slabs, weights_levels, biases_levels, batch, sizes, groups_levels, inside):
    Ps = []
    for x, ws, bs in zip(slabs, weights_levels, biases_levels):
        Wm, bc = pack(ws, bs)
        Ps.append(x @ Wm + bc)
    return permute_restated(Ps, batch, sizes, groups_levels, inside)


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-30))


def scale_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))
