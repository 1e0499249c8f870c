"""CPU: the host side of the up-sampling RPN heads (rpn.strides_anchors, rpn.AnchorNetworkUpsample's anchors, inside mask, dest,
column layout, state-dict keys and loader) against the fixtures the reference's own AnchorNetworkUpsample produced
(tests/golden/make_anchor_up_golden.py), and the torch-operator restatement (tests/anchor_up_restate.py) the GPU tests compare
the kernels with, against the same fixtures: packed weights -> matmul -> permutation reproduces the reference's outputs and
every gradient, which pins the column layout and the anchor order independently of the device.

Bars: the project's fp32 parity bars (README "Parity"): outputs within 1e-4 of the output scale, gradients 2e-5 relative L2."""
import numpy as np
import pytest
import torch

import anchor_up_restate as A

OUT_BAR, GRAD_BAR = 1e-4, 2e-5

# the reference's table (scannet_config/network.py:24-41 on its 3 + 11 anchors, bases 0.6 and 1.2)
STRIDES = (((1, 1, 1), (2, 2, 1)),
           ((1, 1, 1), (1, 1, 3), (1, 2, 1), (1, 4, 1), (1, 6, 1), (2, 1, 1), (3, 3, 1), (4, 1, 1), (6, 1, 1)))
COUNTS = ((2, 1), (2, 2, 1, 1, 1, 1, 1, 1, 1))
ORDERS = ((1, 2, 0), (10, 9, 7, 8, 6, 5, 4, 3, 0, 2, 1))
NCOL = (42, 287)


def test_strides_anchors_reproduces_the_reference_table():
    from sparse_rcnn_amd import rpn as R
    levels = (R.REF_RAW_ANCHORS_M[:3], R.REF_RAW_ANCHORS_M[3:])
    for lv, basis, strides, counts, order in zip(levels, (0.6, 1.2), STRIDES, COUNTS, ORDERS):
        raw = np.asarray(lv)
        groups, got_strides, got_order = R.strides_anchors(lv, basis)
        assert tuple(map(tuple, got_strides.tolist())) == strides
        assert tuple(len(g) for g in groups) == counts
        # the members of every group (their order inside a group is numpy's default argsort's, see strides_anchors)
        o = 0
        for g, n in zip(groups, counts):
            assert sorted(got_order[o:o + n].tolist()) == sorted(order[o:o + n])
            assert np.array_equal(g, raw[got_order[o:o + n]])
            o += n
        # with the recorded order: the recorded groups
        groups, got_strides, got_order = R.strides_anchors(lv, basis, order=order)
        assert got_order.tolist() == list(order) and np.array_equal(np.concatenate(groups), raw[list(order)])
        with pytest.raises(ValueError):
            R.strides_anchors(lv, basis, order=tuple(reversed(order)))
    assert R.REF_UPSAMPLE_ANCHOR_ORDER == ORDERS and R.REF_EXTRA_STRIDE_LEVELS == STRIDES
    # clipping: a maximum folds the large strides together
    _, clipped, _ = R.strides_anchors(levels[1], 1.2, max=2)
    assert int(clipped.max()) == 2 and len(clipped) < len(STRIDES[1])
    # the constants are what the reference's configuration hands to its AnchorNetworkUpsample
    doc = A.keys_doc()
    assert [list(map(list, lv)) for lv in R.REF_EXTRA_STRIDE_LEVELS] == doc["extra_stride_levels"]
    for mine, ref in zip(R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS, doc["anchor_levels_voxels"]):
        assert len(mine) == len(ref)
        for a, b in zip(mine, ref):
            assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("name", A.CASES)
def test_anchors_inside_mask_and_dest_equal_the_reference(name):
    fx = A.fixture(name)
    net = fx.module()
    assert net.ncol_levels == NCOL
    assert net.level_sizes(fx.scene) == tuple(fx.sizes)
    anchors = net.all_anchors(fx.sizes)
    pl = net.plan(fx.scene, fx.sizes, "cpu")
    assert pl.n_all == anchors.shape[0] == fx.inside.shape[0]
    assert torch.equal(pl.inside_cpu, fx.inside)
    assert pl.anchors.dtype == torch.float32 and pl.anchors.numpy().tobytes() == fx.z["inside_anchors"].tobytes()
    assert pl.n_inside == int(fx.inside.sum())
    dest = pl.dest
    assert dest.dtype == torch.int32 and dest.shape[0] == pl.n_all
    assert bool((dest[~fx.inside] == -1).all())
    assert torch.equal(dest[fx.inside].long(), torch.arange(pl.n_inside))
    # the group tables: columns tile [0, Ncol), all-anchor offsets are the running anchor counts
    first = 0
    for (size, ncol, table, n_groups), groups in zip(pl.levels, fx.groups):
        col = 0
        assert n_groups == len(groups)
        for i, ((s0, s1, s2), a) in enumerate(groups):
            assert list(table[6 * i:6 * i + 6]) == [s0, s1, s2, a, col, first]
            col += s0 * s1 * s2 * a * 7
            first += size[0] * size[1] * size[2] * s0 * s1 * s2 * a
        assert col == ncol
    assert first == pl.n_all
    assert net.plan(fx.scene, fx.sizes, "cpu") is pl                                   # kept per (scene shape, sizes, device)
    import pickle
    assert pickle.loads(pickle.dumps(net))._cache == {}                                # and dropped from the pickled state


@pytest.mark.parametrize("name", A.CASES)
def test_restatement_meets_the_reference_outputs_and_gradients(name):
    fx = A.fixture(name)
    net = fx.module()                                                 # its `packed` is the packing the device path uses
    slabs = [fx.slab(l).requires_grad_() for l in range(fx.n_levels)]
    Ps = []
    for l, x in enumerate(slabs):
        Wm, bc = net.packed(l)
        ws = [fx.t(f"w{l}_{k}") for k in range(len(fx.groups[l]))]
        Wr, br = A.pack(ws, [fx.t(f"b{l}_{k}") for k in range(len(fx.groups[l]))])
        assert torch.equal(Wm, Wr) and torch.equal(bc, br) and Wm.shape[1] == NCOL[l]
        s0, s1, s2 = fx.groups[l][-1][0]                              # spot check of the layout: the last tap of the last group
        a7 = fx.groups[l][-1][1] * 7
        assert torch.equal(Wm[:, -a7:], ws[-1][:, :, s0 - 1, s1 - 1, s2 - 1])
        Ps.append(x @ Wm + bc)
    bbox, score = A.permute_restated(Ps, fx.batch, fx.sizes, fx.groups, fx.inside)
    assert tuple(bbox.shape) == tuple(fx.z["rpn_bbox"].shape) and tuple(score.shape) == tuple(fx.z["rpn_score"].shape)
    eb, es = A.scale_err(bbox, fx.t("rpn_bbox")), A.scale_err(score, fx.t("rpn_score"))
    print(f"[anchor up restated] {name}: bbox {eb:.2e} score {es:.2e} of the output scale")
    assert eb <= OUT_BAR and es <= OUT_BAR
    torch.autograd.backward([bbox, score], [fx.t("g_bbox"), fx.t("g_score")])
    for l, x in enumerate(slabs):
        rel = A.rel_l2(x.grad, fx.dslab(l))
        assert rel <= GRAD_BAR, (l, rel)
        for k, h in enumerate(net.rpn_net_levels.operation[l]):
            dw, db = fx.t(f"dw{l}_{k}"), fx.t(f"db{l}_{k}")
            if float(dw.abs().max()) == 0:                            # a group without an inside anchor: exact zeros
                assert float(h.weight.grad.abs().max()) == 0 and float(h.bias.grad.abs().max()) == 0
                continue
            rw, rb = A.rel_l2(h.weight.grad, dw), A.rel_l2(h.bias.grad, db)
            assert rw <= GRAD_BAR and rb <= GRAD_BAR, (l, k, rw, rb)


def test_state_dict_keys_and_loader():
    from sparse_rcnn_amd import rpn as R
    doc = A.keys_doc()
    net = R.AnchorNetworkUpsample(R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS, (4, 8), (128, 256),
                                  extra_stride_levels=R.REF_EXTRA_STRIDE_LEVELS)
    own = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert list(own) == doc["learned"]                                                   # names and order
    assert own == {k: doc["keys"][k] for k in doc["learned"]}                            # shapes: [C, A_g * 7, s0, s1, s2]
    assert own["rpn_net_levels.operation.1.6.weight"] == [256, 7, 3, 3, 1]
    ignored = [k for k in doc["keys"] if k not in doc["learned"]]
    assert ignored and all(k.startswith("anchor_storage.") for k in ignored)
    g = torch.Generator().manual_seed(5)
    ckpt = {k: torch.randn(shape, generator=g) for k, shape in doc["keys"].items()}
    ckpt["anchor_storage.descriptions.x.y"] = torch.zeros(1)
    net.load_reference_state_dict(ckpt)                                                  # bare keys
    assert all(torch.equal(p, ckpt[k]) for k, p in net.named_parameters())
    full = {"bbox_network." + k: v + 1 for k, v in ckpt.items()}
    full["main_network.something.weight"] = torch.zeros(3)                               # the rest of a whole checkpoint
    net.load_reference_state_dict(full)
    assert all(torch.equal(p, ckpt[k] + 1) for k, p in net.named_parameters())
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    bad = dict(ckpt)
    bad["rpn_net_levels.operation.1.2.weight"] = torch.zeros(256, 7, 2, 1, 1)
    with pytest.raises(ValueError, match=r"rpn_net_levels\.operation\.1\.2\.weight"):
        net.load_reference_state_dict(bad)
    extra = dict(ckpt)
    extra["rpn_net_levels.operation.0.2.weight"] = torch.zeros(128, 7, 1, 1, 1)
    with pytest.raises(ValueError, match=r"rpn_net_levels\.operation\.0\.2\.weight"):
        net.load_reference_state_dict(extra)
    lacking = {k: v for k, v in ckpt.items() if k != "rpn_net_levels.operation.1.8.bias"}
    with pytest.raises(ValueError, match=r"rpn_net_levels\.operation\.1\.8\.bias"):
        net.load_reference_state_dict(lacking)
    assert all(torch.equal(p, before[k]) for k, p in net.named_parameters())              # a refused checkpoint copies nothing


def test_no_cpu_fallback():
    import sparse_rcnn_amd as scn
    from sparse_rcnn_amd import rpn as R
    fx = A.fixture("border")
    net = fx.module()
    slabs = [(fx.slab(l), fx.sizes[l], fx.batch) for l in range(fx.n_levels)]
    with pytest.raises(scn.ScnError, match="no CPU fallback"):
        net(slabs, fx.scene)
    with pytest.raises(scn.ScnError):
        from sparse_rcnn_amd.functional import AnchorUpFunction
        pl = net.plan(fx.scene, fx.sizes, "cpu")
        AnchorUpFunction.apply(pl, fx.batch, *[torch.zeros(s[0].shape[0], n) for s, n in zip(slabs, net.ncol_levels)])
    # the module layout of MultiLevelRpn: without extra strides exactly the 1x1 heads, with them no per-level head
    levels = [(8, 4, 8, R.REF_ANCHOR_LEVELS_VOXELS[0]), (8, 8, 8, R.REF_ANCHOR_LEVELS_VOXELS[1])]
    torch.manual_seed(3)
    plain = R.MultiLevelRpn(levels, num_dilations=1)
    assert plain.anchor_network is None and [k for k, _ in plain.named_parameters()] == [
        "levels.0.stack.0.weight", "levels.0.stack.0.bias", "levels.0.head.weight", "levels.0.head.bias",
        "levels.1.stack.0.weight", "levels.1.stack.0.bias", "levels.1.head.weight", "levels.1.head.bias"]
    up_levels = [(8, 4, 8, R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS[0]), (8, 8, 8, R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS[1])]
    up = R.MultiLevelRpn(up_levels, num_dilations=1, extra_stride_levels=R.REF_EXTRA_STRIDE_LEVELS)
    names = [k for k, _ in up.named_parameters()]
    assert not any(".head." in k for k in names) and all(l.head is None for l in up.levels)
    assert [k for k in names if k.startswith("anchor_network.")] == ["anchor_network." + k for k in A.keys_doc()["learned"]]
