"""CPU: the anchor bookkeeping of the RPN boundary (rpn.py) against fixtures produced by the reference's own
AnchorDescriptionMultiLevel (ndsis/modules/anchor.py:57-227; tests/golden/make_anchor_golden.py): pixel-wise anchors in
spatial-major / anchor-minor order, the inside-the-scene indicator (`allowed_border`), the compaction of head outputs
(`rpn_permuter` + `rpn_bbox_score_splitter`) and the decode + clip of `forward` -- bit for bit."""
import os

import numpy as np
import pytest
import torch

from sparse_rcnn_amd import rpn as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    return np.load(os.path.join(GOLD, f"anchor_{name}.npz"))


def _raw_of_head(head, n_anchors):
    """[B, A * 7, X, Y, Z] -> [B, X Y Z A, 7]: what DenseRpn.forward hands to `_finish` (spatial-major, anchor-minor)."""
    B = head.shape[0]
    return head.view(B, n_anchors, 7, -1).permute(0, 3, 1, 2).reshape(B, -1, 7)


@pytest.mark.parametrize("name", ["one_level", "border"])
def test_single_level_anchors_inside_mask_and_compaction_equal_the_reference(name):
    g = _load(name)
    stride, border = int(g["strides"][0]), float(g["border"])
    anchors = [tuple(map(float, a)) for a in g["anchors0"]]
    shape = tuple(int(v) for v in g["conv_shape0"])
    rpn = R.DenseRpn(8, stride=stride, width=8, num_dilations=1, anchors=anchors, allowed_border=border)
    a = rpn.anchors_for(shape, "cpu")
    ind = R.inside_indicator(a, torch.from_numpy(g["scene_shape"]).float(), border)
    assert np.array_equal(ind.numpy(), g["inside_indicator"])
    idx, inside = rpn.inside_for(shape, "cpu")
    assert torch.equal(idx, ind.nonzero().squeeze(1)) and np.array_equal(inside.numpy(), g["inside_anchors"])
    assert 0 < len(idx) < len(a)
    bbox, score, anch = rpn._finish(_raw_of_head(torch.from_numpy(g["head0"]), len(anchors)), shape)
    assert np.array_equal(bbox.numpy(), g["rpn_bbox"]) and np.array_equal(score.numpy(), g["rpn_score"])
    assert np.array_equal(anch.numpy(), g["inside_anchors"])
    boxes = R.decode_boxes(anch, bbox, tuple(float(v) for v in g["scene_shape"]))
    assert np.array_equal(boxes.numpy(), g["boxes"])
    unclipped = R.decode_boxes(anch, bbox)
    assert (unclipped != boxes).any()                       # the fixture does clip something


def test_two_anchor_levels_concatenate_and_compact_like_the_reference():
    g = _load("two_levels")
    levels = []
    for l in range(int(g["n_levels"])):
        levels.append((8, int(g["strides"][l]), 8, [tuple(map(float, a)) for a in g[f"anchors{l}"]]))
    m = R.MultiLevelRpn(levels, num_dilations=1)
    outs = []
    for l, rpn in enumerate(m.levels):
        shape = tuple(int(v) for v in g[f"conv_shape{l}"])
        assert not rpn.keep_inside
        outs.append(rpn._finish(_raw_of_head(torch.from_numpy(g[f"head{l}"]), rpn.n_anchors), shape))
    scene = tuple(int(v) for v in g["scene_shape"])
    bbox, score, anch = m.combine(outs, scene)
    assert np.array_equal(anch.numpy(), g["inside_anchors"])
    assert np.array_equal(bbox.numpy(), g["rpn_bbox"]) and np.array_equal(score.numpy(), g["rpn_score"])
    assert np.array_equal(R.decode_boxes(anch, bbox, tuple(float(v) for v in scene)).numpy(), g["boxes"])
    # the reference's anchor table in voxels (scannet_config/network.py:7-23 at 0.0375 m): 3 small + 11 large
    assert [len(a) for a in R.REF_ANCHOR_LEVELS_VOXELS] == [3, 11]
    assert np.allclose(R.REF_ANCHOR_LEVELS_VOXELS[0][0], np.array([0.3752, 0.3752, 0.4221]) / 0.0375)


def test_roi_selector_raises_on_rows_outside_the_volume():
    sel = R.RoiSelector(4, 2, 0.5)
    flag = torch.ones(1, dtype=torch.int32)

    class _PS(torch.nn.Module):     # the selection itself needs the GPU library; the flag check is host logic
        def finish(self, st):
            return ([], [], [])
    sel.proposal_selector = _PS()
    with pytest.raises(Exception, match="outside its spatial_size"):
        sel.finish((None, None, None, None, [flag]))
    assert sel.finish((None, None, None, None, [torch.zeros(1, dtype=torch.int32)])) == ([], [], [])


def test_get_roi_selector_follows_training_mode_like_the_references_conditional_stage():
    """proposal_selector.py:6-20 / custom_container.py:102-116: one selector, or a train / eval pair chosen by `.training`
    (scannet_config/run.py:847-853: 1024 / 256 / 0.5 against 1024 / 32 / 0.3)."""
    one = R.get_roi_selector(1024, 256, 0.5)
    assert isinstance(one, R.RoiSelector) and one.proposal_selector.num_keep_post_nms == 256
    pair = R.get_roi_selector(1024, 256, 0.5, val_num_keep_pre_nms=1024, val_num_keep_post_nms=32, val_thresh_nms=0.3)
    assert pair._member().proposal_selector.num_keep_post_nms == 256 and pair._member().proposal_selector.thresh_nms == 0.5
    pair.eval()
    assert pair._member().proposal_selector.num_keep_post_nms == 32 and pair._member().proposal_selector.thresh_nms == 0.3
    pair.train()
    assert pair._member() is pair.train_module


# ---- the dense stack's oracle (oracle.scn_oracle.dense_rpn_forward): the GPU tests hold DenseRpn's "tiles" engine to it
def _level(seed, size, batch, n, c, empty=()):
    """n random active cells per sample (none in the samples of `empty`) of a `size` grid, features [rows, c]."""
    rng = np.random.default_rng(seed)
    cs = []
    for b in range(batch):
        if b in empty:
            continue
        lin = rng.choice(int(np.prod(size)), size=n, replace=False)
        cs.append(np.concatenate([np.stack(np.unravel_index(lin, size), 1), np.full((n, 1), b)], 1))
    coords = np.concatenate(cs).astype(np.int64)
    X = torch.randn(len(coords), c, generator=torch.Generator().manual_seed(seed + 1))
    return coords, X


def _cpu_rpn(c, width, n_dil, seed=3):
    torch.manual_seed(seed)
    net = R.DenseRpn(c, stride=8, width=width, num_dilations=n_dil, keep_inside=False)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn_like(p) * 0.1)
    convs = [l for l in net.stack if isinstance(l, torch.nn.Conv3d)]
    return net, [(l.weight, l.bias) for l in convs], (net.head.weight, net.head.bias)


def _scale_err(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("c,width,size,batch", [(16, 16, (7, 6, 5), 2), (24, 8, (5, 4, 3), 3), (20, 16, (6, 5, 4), 2)])
def test_dense_rpn_oracle_both_first_layer_forms_equal_torch_conv3d(c, width, size, batch):
    """With identity roundings the sparse first layer (row GEMM + dilation gather, zero padding at the faces) and the dense
    one both equal the module's own `head(stack(sparse_to_dense(X)))` within fp32 rounding, forward and every gradient."""
    from oracle import scn_oracle as O
    net, stack, head = _cpu_rpn(c, width, 2)
    coords, X = _level(1, size, batch, 20, c)
    X.requires_grad_()
    ref = net.head(net.stack(O.sparse_to_dense(X, coords, size, batch)))
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(2))
    params = list(net.parameters())
    ref_g = torch.autograd.grad(ref, [X] + params, g)
    for sparse_first in (True, False):
        got = O.dense_rpn_forward(X, coords, size, batch, stack, head, sparse_first=sparse_first)
        assert got.shape == ref.shape and _scale_err(got, ref) <= 1e-6, sparse_first
        for a, b in zip(torch.autograd.grad(got, [X] + params, g), ref_g):
            assert _scale_err(a, b) <= 1e-6, sparse_first


def test_dense_rpn_oracle_bf16_roundings_of_the_two_forms_agree_within_bf16_noise():
    """The bf16 storage roundings (P and every stored layer output rounded, tile-kernel weights rounded in the dense form
    only) move the output by bf16 noise, and the two forms land within that noise of each other; with a level width that is
    not a multiple of 8 the stack is widened to fp32 before its first layer and no rounding is left."""
    from oracle import scn_oracle as O
    r = O.bf16_storage
    for c, width, sparse_diff in ((16, 16, True), (20, 16, False)):
        net, stack, head = _cpu_rpn(c, width, 3)
        coords, X = _level(4, (8, 7, 5), 2, 40, c)
        X = X.to(torch.bfloat16).float()                          # a bf16-stored level
        with torch.no_grad():
            f32 = O.dense_rpn_forward(X, coords, (8, 7, 5), 2, stack, head)
            outs = [O.dense_rpn_forward(X, coords, (8, 7, 5), 2, stack, head, storage=r, tile_weights=r, sparse_first=sf)
                    for sf in (True, False)]
        for o in outs:
            if sparse_diff:
                assert 1e-5 < _scale_err(o, f32) <= 2.0 ** -6
            else:
                assert torch.equal(o, f32)
        e = _scale_err(outs[0], outs[1])
        assert (0 < e <= 2.0 ** -6) if sparse_diff else e == 0
        assert float((outs[0] - outs[1]).norm() / outs[1].norm()) <= 1e-2


@pytest.mark.parametrize("sparse_first", [True, False])
def test_dense_rpn_oracle_of_an_empty_sample_is_the_head_of_the_bias_only_stack(sparse_first):
    """A sample without active rows sees the bias of the first layer on every cell; the rest of the stack and the head then
    act on that constant volume as on any other -- exactly, since adding zeros changes no bit (the reference runs the whole
    batch, every sample at the bias, so that torch's CPU convolution blocks the batch the same way)."""
    from oracle import scn_oracle as O
    net, stack, head = _cpu_rpn(16, 8, 3)
    size = (6, 5, 4)
    coords, X = _level(7, size, 3, 15, 16, empty=(1,))
    got = O.dense_rpn_forward(X, coords, size, 3, stack, head, sparse_first=sparse_first)
    with torch.no_grad():
        h = stack[0][1].view(1, -1, 1, 1, 1).expand(3, -1, *size).contiguous()
        for W, b in stack[1:]:
            h = torch.nn.functional.conv3d(torch.relu(h), W, b, padding=1)
        exp = torch.nn.functional.conv3d(torch.relu(h), *head)
    assert torch.equal(got[1].detach(), exp[1])
    assert not torch.equal(got[0], got[1])
