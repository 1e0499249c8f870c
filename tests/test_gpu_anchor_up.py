"""MI355X: the up-sampling RPN heads -- the two kernels (scn_anchor_up_fwd / _bwd) alone against the torch-operator
restatement (tests/anchor_up_restate.py, pinned to the reference's fixtures by tests/test_anchor_up_cpu.py), the head
(rpn.AnchorNetworkUpsample: row GEMM + scatter) against the fixtures the reference's own AnchorNetworkUpsample produced
(tests/golden/make_anchor_up_golden.py), MultiLevelRpn with and without the heads, and the step that uses them.

Bars: the kernels only copy -- bit-equal.  The head: the project's fp32 parity bars (README "Parity"), outputs within 1e-4 of the
output scale, every gradient within 2e-5 relative L2."""
import numpy as np
import pytest
import torch

import anchor_up_restate as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
OUT_BAR, GRAD_BAR = 1e-4, 2e-5
GUARD = 777.0


def _ref_module(scale=1.0, channels=(128, 256), border=0):
    from sparse_rcnn_amd import rpn as R
    anchors = [[np.asarray(g) * scale for g in lv] for lv in R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS]
    return R.AnchorNetworkUpsample(anchors, (4, 8), channels, border, extra_stride_levels=R.REF_EXTRA_STRIDE_LEVELS)


def _shape(name):
    """-> (module, scene, level sizes, batch, groups per level, inside mask)"""
    if name == "crop":                      # one sample of the reference's crop: P 16 384 x 42 and 2 048 x 287
        net, scene, batch = _ref_module(), (128, 128, 64), 1
        sizes = net.level_sizes(scene)
        assert [s[0] * s[1] * s[2] for s in sizes] == [16384, 2048]
    else:
        fx = A.fixture(name)
        net, scene, batch, sizes = fx.module(), fx.scene, fx.batch, fx.sizes
    groups = [[(g["extra"], g["n_anchors"]) for g in lv] for lv in net._groups]
    pl = net.plan(scene, sizes, DEV)
    return net, pl, sizes, batch, groups


def _guarded(n):
    buf = torch.full((n + 128,), GUARD, dtype=torch.float32, device=DEV)
    return buf, buf[64:64 + n]


def _intact(buf):
    return bool((buf[:64] == GUARD).all()) and bool((buf[-64:] == GUARD).all())


@pytest.mark.parametrize("name", list(A.CASES) + ["crop"])
def test_kernels_bit_equal_to_the_restated_permutation(name):
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.functional import _host3
    lib = L.lib()
    net, pl, sizes, batch, groups = _shape(name)
    if name == "crop":
        assert (pl.n_all, pl.n_inside) == (182272, 88536)
    g = torch.Generator().manual_seed(7)
    Ps = [torch.randn((batch * s[0] * s[1] * s[2], ncol), generator=g).to(DEV) for s, ncol in zip(sizes, net.ncol_levels)]
    inside = pl.inside_cpu
    ref_bbox, ref_score = A.permute_restated(Ps, batch, sizes, groups, inside)
    # forward, both levels into guarded outputs
    bbuf, bbox = _guarded(batch * pl.n_inside * 6)
    sbuf, score = _guarded(batch * pl.n_inside)
    bbox.fill_(float("nan"))
    score.fill_(float("nan"))
    for P, (size, ncol, table, ng) in zip(Ps, pl.levels):
        L.check(lib.scn_anchor_up_fwd(L.ptr(P), batch, _host3(size), ncol, table, ng, L.ptr(pl.dest), pl.n_all, pl.n_inside,
                                      L.ptr(bbox), L.ptr(score), L.stream()))
    torch.cuda.synchronize()
    assert _intact(bbuf) and _intact(sbuf)
    assert torch.equal(bbox.view(batch, pl.n_inside, 2, 3), ref_bbox) and torch.equal(score.view(batch, pl.n_inside), ref_score)
    # backward: dP pre-filled with NaN, every element written; the restatement is autograd through the torch permutation
    d_bbox = torch.randn(ref_bbox.shape, generator=g).to(DEV)
    d_score = torch.randn(ref_score.shape, generator=g).to(DEV)
    leaves = [P.clone().requires_grad_() for P in Ps]
    rb, rs = A.permute_restated(leaves, batch, sizes, groups, inside)
    torch.autograd.backward([rb, rs], [d_bbox, d_score])
    leaves_b = [P.clone().requires_grad_() for P in Ps]
    rb, _ = A.permute_restated(leaves_b, batch, sizes, groups, inside)
    rb.backward(d_bbox)
    o = 0
    for l, (P, (size, ncol, table, ng)) in enumerate(zip(Ps, pl.levels)):
        runs = []
        for ds in (d_score, d_score, None):
            dbuf, dP = _guarded(P.numel())
            dP.fill_(float("nan"))
            L.check(lib.scn_anchor_up_bwd(L.ptr(d_bbox), L.ptr(ds), batch, _host3(size), ncol, table, ng, L.ptr(pl.dest), pl.n_all,
                                          pl.n_inside, L.ptr(dP), L.stream()))
            torch.cuda.synchronize()
            assert _intact(dbuf)
            runs.append(dP.view(P.shape))
        assert not bool(torch.isnan(runs[0]).any())                                   # every element written
        assert torch.equal(runs[0], leaves[l].grad)
        assert torch.equal(runs[0], runs[1])                                          # a second run: the same bits
        assert torch.equal(runs[2], leaves_b[l].grad)                                 # d_score absent = zeros
        # anchors outside the scene: exact zeros
        n_level = sum(size[0] * size[1] * size[2] * e[0] * e[1] * e[2] * a for e, a in groups[l])
        outside = ~inside[o:o + n_level]
        o += n_level
        rec = A.all_records(runs[0], batch, size, groups[l])
        assert bool((rec[:, outside.to(DEV)] == 0).all())
    assert o == pl.n_all


def test_bad_arguments_are_refused_before_any_launch():
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.functional import _host3
    lib = L.lib()
    net, pl, sizes, batch, groups = _shape("border")
    size, ncol, table, ng = pl.levels[1]
    P = torch.zeros((batch * size[0] * size[1] * size[2], ncol), device=DEV)
    bbox = torch.full((batch, pl.n_inside, 2, 3), GUARD, device=DEV)
    score = torch.full((batch, pl.n_inside), GUARD, device=DEV)

    def call(**kw):
        a = dict(P=L.ptr(P), batch=batch, size=_host3(size), ncol=ncol, table=table, ng=ng, dest=L.ptr(pl.dest), n_all=pl.n_all,
                 n_inside=pl.n_inside)
        a.update(kw)
        return lib.scn_anchor_up_fwd(a["P"], a["batch"], a["size"], a["ncol"], a["table"], a["ng"], a["dest"], a["n_all"],
                                     a["n_inside"], L.ptr(bbox), L.ptr(score), L.stream())
    gap = L.host_i64(6 * ng)
    gap[:] = list(table)
    gap[4] = 7                                                        # the first group's columns do not start at 0
    short = L.host_i64(6 * ng)
    short[:] = list(table)
    short[6 * (ng - 1) + 5] = pl.n_all                                # the last group's anchors leave dest
    for kw in (dict(P=0), dict(dest=0), dict(ncol=ncol + 1), dict(ncol=ncol - 7), dict(ng=0), dict(ng=L.ANCHOR_UP_MAX_GROUPS + 1),
               dict(size=_host3((size[0], 0, size[2]))), dict(n_inside=pl.n_all + 1), dict(batch=-1), dict(table=gap),
               dict(table=short), dict(n_all=pl.n_all - 1)):
        assert call(**kw) == L.EINVAL, kw
    torch.cuda.synchronize()
    assert bool((bbox == GUARD).all()) and bool((score == GUARD).all())
    assert call() == L.OK


@pytest.mark.parametrize("name", A.CASES)
def test_head_against_the_reference_fixture(name):
    fx = A.fixture(name)
    net = fx.module().to(DEV)
    slabs = [fx.slab(l).to(DEV).requires_grad_() for l in range(fx.n_levels)]
    bbox, score, anchors = net([(x, fx.sizes[l], fx.batch) for l, x in enumerate(slabs)], fx.scene)
    assert anchors.cpu().numpy().tobytes() == fx.z["inside_anchors"].tobytes()
    assert bbox.is_contiguous() and score.is_contiguous()
    assert tuple(bbox.shape) == tuple(fx.z["rpn_bbox"].shape) and tuple(score.shape) == tuple(fx.z["rpn_score"].shape)
    eb, es = A.scale_err(bbox, fx.t("rpn_bbox")), A.scale_err(score, fx.t("rpn_score"))
    print(f"[anchor up head] {name}: rpn_bbox {eb:.2e} rpn_score {es:.2e} of the output scale")
    assert eb <= OUT_BAR and es <= OUT_BAR
    torch.autograd.backward([bbox, score], [fx.t("g_bbox").to(DEV), fx.t("g_score").to(DEV)])
    worst = 0.0
    for l, x in enumerate(slabs):
        rel = A.rel_l2(x.grad, fx.dslab(l))
        print(f"[anchor up head] {name}: d volume {l} rel L2 {rel:.2e}")
        assert rel <= GRAD_BAR, (l, rel)
        worst = max(worst, rel)
        for k, h in enumerate(net.rpn_net_levels.operation[l]):
            dw, db = fx.t(f"dw{l}_{k}"), fx.t(f"db{l}_{k}")
            if float(dw.abs().max()) == 0:                            # a group without an inside anchor: exact zeros
                assert float(h.weight.grad.abs().max()) == 0 and float(h.bias.grad.abs().max()) == 0
                continue
            rw, rb = A.rel_l2(h.weight.grad, dw), A.rel_l2(h.bias.grad, db)
            assert rw <= GRAD_BAR and rb <= GRAD_BAR, (l, k, rw, rb)
            worst = max(worst, rw, rb)
    print(f"[anchor up head] {name}: worst gradient rel L2 {worst:.2e}")
    # the head of one level alone: only rpn_score asked for (d_bbox absent)
    for x in slabs:
        x.grad = None
    bbox, score, _ = net([(x, fx.sizes[l], fx.batch) for l, x in enumerate(slabs)], fx.scene)
    score.sum().backward()
    assert all(x.grad is not None and bool(torch.isfinite(x.grad).all()) for x in slabs)


# The smallest grid the workload accepts: a multiple of 2^5 per axis (the 6-level plan) that holds the 1024 inside anchors the
# selector's top-k asks for, as the reference's does (32^3: 696; this one: 1864 per crop).  12 crops as the workload has.
GRID, TARGET = (64, 32, 32), 3000


def _step(upsample, seed=1, **kw):
    from sparse_rcnn_amd.trainstep import SceneStep
    return SceneStep("ref-crop-rpn", grid=GRID, target=TARGET, prefetch=False, seed=seed,
                     **(dict(upsample_heads=True) if upsample else {}), **kw)


def _levels(st):
    m = st.model
    with torch.no_grad():
        m.backbone(st.coords, st.feats, st.size, st.batch_size, metadata=None)
    return [m.backbone.unet.interims[i] for i in m.rpn_levels]


def test_multilevel_rpn_without_extra_strides_is_the_parent():
    """extra_stride_levels=None: the modules, their order, their seeded values and the outputs are those of the composition
    this change found -- DenseRpn levels (constructed with the argument list MultiLevelRpn used) + concatenation + inside mask."""
    from sparse_rcnn_amd import rpn as R
    st = _step(False)
    lv = _levels(st)
    levels = [(st.channels[2], 4, 128, R.REF_ANCHOR_LEVELS_VOXELS[0]), (st.channels[3], 8, 256, R.REF_ANCHOR_LEVELS_VOXELS[1])]
    torch.manual_seed(11)
    mine = R.MultiLevelRpn(levels, num_dilations=5).to(DEV)
    torch.manual_seed(11)
    hand = torch.nn.ModuleList(R.DenseRpn(c, stride, width, 5, tuple(map(tuple, a)), False, None, keep_inside=False,
                                          keep_volume=False) for c, stride, width, a in levels).to(DEV)
    assert mine.anchor_network is None
    assert [k for k, _ in mine.named_parameters()] == ["levels." + k for k, _ in hand.named_parameters()]
    assert all(torch.equal(a, b) for a, b in zip(mine.parameters(), hand.parameters()))
    with torch.no_grad():
        bbox, score, anchors = mine(lv)
        outs = [r(t) for r, t in zip(hand, lv)]
    all_anchors = torch.cat([o[2] for o in outs], 0)
    idx = R.inside_indicator(all_anchors, torch.tensor(GRID, dtype=torch.float32)).nonzero().squeeze(1)
    assert idx.numel() > 0
    assert torch.equal(bbox, torch.cat([o[0] for o in outs], 1).index_select(1, idx))
    assert torch.equal(score, torch.cat([o[1] for o in outs], 1).index_select(1, idx))
    assert torch.equal(anchors, all_anchors[idx])
    assert len(score.cell_flags) == 2
    st.finish()


def test_multilevel_rpn_with_the_heads_keeps_the_volume_for_the_dense_class_branch():
    from sparse_rcnn_amd import rpn as R
    from sparse_rcnn_amd.classhead import DenseClassBranch
    st = _step(False)
    lv = _levels(st)
    levels = [(st.channels[2], 4, 128, R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS[0]),
              (st.channels[3], 8, 256, R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS[1])]
    torch.manual_seed(12)
    rpn = R.MultiLevelRpn(levels, num_dilations=5, keep_volume=True, extra_stride_levels=R.REF_EXTRA_STRIDE_LEVELS).to(DEV)
    bbox, score, anchors = rpn(lv)
    B = st.batch_size
    calc = rpn.target_calculator(GRID)
    assert torch.equal(calc.anchors, anchors) and calc.anchors.data_ptr() == anchors.data_ptr()      # one tensor, kept
    n = anchors.shape[0]
    assert n > 0 and tuple(bbox.shape) == (B, n, 2, 3) and tuple(score.shape) == (B, n)
    assert len(score.cell_flags) == 2 and all(int(f[0]) == 0 for f in score.cell_flags)
    # the restated head on the kept slabs: what the scatter wrote is the permutation of the row GEMM
    slab, size, batch, md = rpn.volume
    assert tuple(size) == (16, 8, 8) and batch == B and tuple(slab.shape) == (B * 1024, 128)
    branch = DenseClassBranch(128, 4).to(DEV)
    boxes = [b[:4].float().to(DEV) for b in st.gt_boxes]
    scores, _ = branch(slab, size, batch, boxes, metadata=md)
    w = rpn.levels[0].stack[0].weight
    (gw,) = torch.autograd.grad(scores.sum() + score.sum(), [w])
    assert scores.shape == (4 * B, 18) and bool(torch.isfinite(gw).all()) and float(gw.abs().sum()) > 0
    st.finish()


def test_scenestep_with_the_upsampling_heads():
    kw = dict(rpn_loss=True, mask_loss=True, class_loss=True, dense_class=True, segmentation_loss=True, optimizer="adam", n_gt=8)
    runs = []
    for _ in range(2):
        st = _step(True, **kw)
        d = st.describe()
        assert "AnchorNetworkUpsample heads" in d and "1x1 head" not in d
        up = st.model.rpn.anchor_network
        assert up is not None and all(l.head is None for l in st.model.rpn.levels)
        st.keep_rpn_grads = True
        st.step()
        losses = [float(v.detach().cpu()) for v in (*st.rpn_losses, st.mask_losses, st.class_losses, st.segmentation_losses)]
        print("[anchor up step] losses (rpn score, rpn bbox, mask, class, segmentation):", " ".join(f"{v:.5f}" for v in losses))
        assert np.isfinite(losses).all()
        pl = up.plan(tuple(float(v) for v in GRID), up.level_sizes(GRID), st.device)
        rpn_bbox, rpn_score = st.rpn_out[:2]
        assert tuple(rpn_score.shape) == (st.batch_size, pl.n_inside) and pl.n_inside == 1864
        # Per group: its inside anchors (a range of ranks) and whether the loss sent a gradient to any of them.  With the
        # reference's anchor sizes this scene holds anchors of three groups only: the other eight are empty inside a real step.
        # Every head parameter has a gradient; it is non-zero where a gradient reached the group's anchors and exactly zero
        # where none did (an empty group, or one the draw passed over).
        reached = (rpn_score.grad != 0) | (rpn_bbox.grad != 0).flatten(2).any(2)
        o, r0, n_in, hit = 0, 0, [], []
        for groups, size in zip(up._groups, up.level_sizes(GRID)):
            for g in groups:
                n = size[0] * size[1] * size[2] * g["extra"][0] * g["extra"][1] * g["extra"][2] * g["n_anchors"]
                k = int(pl.inside_cpu[o:o + n].sum())
                n_in.append(k)
                hit.append(bool(reached[:, r0:r0 + k].any()))
                o, r0 = o + n, r0 + k
        print("[anchor up step] inside anchors per group", n_in, "gradient reached", hit)
        assert n_in == [288, 1560, 0, 0, 16, 0, 0, 0, 0, 0, 0]
        assert hit == [True, True, False, False, True] + [False] * 6        # (seeded: the draw reaches the 16-anchor group too)
        for h, alive in zip(up.heads(), hit):
            for p in (h.weight, h.bias):
                assert p.grad is not None and bool(torch.isfinite(p.grad).all())
                assert (float(p.grad.abs().sum()) > 0) == alive
        out = st.predict()
        st.finish()
        assert {"roi_bbox", "class", "mask", "segmentation_class"} <= set(out)
        runs.append((losses, st.flat.flat.detach().clone(), torch.cat([b.reshape(-1) for b in out["roi_bbox"]]).clone()))
        del st
    assert runs[0][0] == runs[1][0]                                        # two equally seeded runs: the same bits
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    # the default step is untouched by the switch's existence
    plain = _step(False, rpn_loss=True)
    d = plain.describe()
    assert "1x1 head" in d and "upsample_heads=True" in d and plain.model.rpn.anchor_network is None
    plain.finish()
    from sparse_rcnn_amd.trainstep import SceneStep
    with pytest.raises(ValueError, match="ref-crop-rpn"):
        SceneStep("cfg3-rpn", upsample_heads=True)
