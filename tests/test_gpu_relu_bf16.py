"""MI355X: the stand-alone ReLU on a bf16-stored slab (scn_relu_fwd_bf16 / scn_relu_bwd_bf16) and what it opens up -- the
reference's up-sampling RPN heads behind a bf16-stored dilation stack.

Everything here is an EQUALITY, no tolerance:
  * the entry points against their fp32 twins (scn_relu_fwd / scn_relu_bwd) run on the widened inputs on the same GPU, compared
    as bit patterns (the twins' results are bf16 values, so narrowing them is taking their upper 16 bits);
  * functional.ReLUFunction on bf16 against itself on the widened tensor;
  * MultiLevelRpn with the heads on bf16 level tensors against the fp32-tail twin: the same bf16 stack output, widened, the fp32
    ReLUFunction, the same heads.  Forward: widen(relu_bf16(x)) == relu(widen(x)).  Backward: the twin masks the fp32 gradient and
    rounds it once (the backward of .float()), the new path rounds once and masks; masking selects the value or +0 and rounding
    maps 0 to 0, so every gradient is the same bits;
  * two equally seeded steps.
Confirmed by hand before this file was committed: with `>=` for `>` in k_relu_b's backward the raw test fails at the +-0 specials."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
EW_THREADS = 2048 * 256          # scn::ew_grid: at most 2048 blocks of 256 threads, then the loop strides
COUNTS = [0, 1, 7, 8, 9, 2047, 2048, 2049, 8 * EW_THREADS + 8 * 300 + 5]      # the last: a second trip at 8 elements per thread
GUARD, SENT = 512, 0xA5
# +-0, +-inf, NaN (quiet; negative with a payload), largest and smallest denormals of both signs, +-smallest normal
SPECIALS = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x007F, 0x807F, 0x0001, 0x8001, 0x0080, 0x8080]


def _L():
    from sparse_rcnn_amd import _lib as L
    return L


class Buf:
    """`count` int16 elements (bf16 bit patterns) or floats inside a sentinel-filled byte buffer; the data starts `off` elements
    past a 256-byte boundary.  `.t` views the data, `.intact()` says whether every byte outside it is untouched."""

    def __init__(self, dtype, count, off=0, fill=None):
        isz = torch.empty((), dtype=dtype).element_size()
        self.lo = GUARD + off * isz
        self.hi = self.lo + int(count) * isz
        self.raw = torch.full((self.hi + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 256 == 0
        self.t = self.raw[self.lo:self.hi].view(dtype)
        if fill is not None:
            self.t.copy_(fill.reshape(-1))
        self.ptr = self.raw.data_ptr() + self.lo

    def intact(self):
        return bool((self.raw[:self.lo] == SENT).all()) and bool((self.raw[self.hi:] == SENT).all())


def _bits16(n, seed, shift):
    """int16 bit patterns of randn rounded to bf16, with SPECIALS at the positions i with (i + shift) % 37 < 12 (two operands with
    shifts 0 and 17 never hold a special at the same position: a +-0 input meets an ordinary non-zero gradient)."""
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).view(torch.int16)
    k = (torch.arange(n) + shift) % 37
    m = k < len(SPECIALS)
    x[m] = torch.tensor(SPECIALS, dtype=torch.int32).to(torch.int16)[k[m]]       # (wraps to the same 16 bits)
    return x


def _widen(b):
    """int16 bf16 bit patterns -> the fp32 tensor of the same values, NaN payloads included."""
    return (b.to(torch.int32) << 16).view(torch.float32)


def _narrow(f):
    """fp32 tensor of bf16 VALUES -> their int16 bit patterns; the lower 16 bits must be clear."""
    i = f.contiguous().view(torch.int32)
    assert bool(((i & 0xFFFF) == 0).all())
    return (i >> 16).to(torch.int16)


@pytest.fixture(scope="module")
def operands():
    n = COUNTS[-1]
    return _bits16(n, 1, 0).to(DEV), _bits16(n, 2, 17).to(DEV)


# ---- 1. the raw entry points -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
def test_entry_points_equal_the_fp32_twins_on_widened_inputs(operands, bwd):
    """All pointers 16-byte aligned (uint4 body + scalar tail) and each pointer in turn one element off (scalar body); counts
    around the lane width, around the block, and one that sends the vector body round its loop a second time with a tail of 5."""
    L = _L()
    lib = L.lib()
    X, G = operands
    offs = [(0, 0, 0), (1, 0, 0), (0, 0, 1)] + ([(0, 1, 0)] if bwd else [])
    for count, (ox, og, oy) in itertools.product(COUNTS, offs):
        x, g = Buf(torch.int16, count, ox, X[:count]), Buf(torch.int16, count, og, G[:count])
        xw, gw, ref = Buf(torch.float32, count, 0, _widen(x.t)), Buf(torch.float32, count, 0, _widen(g.t)), Buf(torch.float32, count)
        runs = []
        for _ in range(2):
            y = Buf(torch.int16, count, oy)
            if bwd:
                L.check(lib.scn_relu_bwd_bf16(x.ptr, g.ptr, count, y.ptr, L.stream()))
            else:
                L.check(lib.scn_relu_fwd_bf16(x.ptr, count, y.ptr, L.stream()))
            assert y.intact() and x.intact() and g.intact(), ("guard", count, ox, og, oy)
            runs.append(y.t)
        if bwd:
            L.check(lib.scn_relu_bwd(xw.ptr, gw.ptr, count, ref.ptr, L.stream()))
        else:
            L.check(lib.scn_relu_fwd(xw.ptr, count, ref.ptr, L.stream()))
        want = _narrow(ref.t)
        assert torch.equal(runs[0], want), (count, ox, og, oy, (runs[0] != want).nonzero()[:8].flatten().tolist())
        assert torch.equal(runs[0], runs[1]), (count, ox, og, oy)
    # the contract in words on the first six specials (+0, -0, +inf, -inf, NaN, -NaN; the denormals follow the twin above):
    # only +inf passes anything, everything else gives +0 whatever the (ordinary, non-zero) gradient holds
    n = 6
    x, g, y = Buf(torch.int16, n, 0, X[:n]), Buf(torch.int16, n, 0, G[:n]), Buf(torch.int16, n)
    assert bool((g.t != 0).all())
    if bwd:
        L.check(lib.scn_relu_bwd_bf16(x.ptr, g.ptr, n, y.ptr, L.stream()))
        assert y.t.tolist() == [0, 0, int(g.t[2]), 0, 0, 0]
    else:
        L.check(lib.scn_relu_fwd_bf16(x.ptr, n, y.ptr, L.stream()))
        assert y.t.tolist() == [0, 0, 0x7F80, 0, 0, 0]


def test_status_codes_come_before_any_launch():
    L = _L()
    lib = L.lib()
    x = torch.zeros(16, dtype=torch.int16, device=DEV)
    y = torch.full((16,), 0x5A5A, dtype=torch.int16, device=DEV)
    s = L.stream()
    assert lib.scn_relu_fwd_bf16(0, 0, 0, s) == L.OK and lib.scn_relu_bwd_bf16(0, 0, 0, 0, s) == L.OK
    assert lib.scn_relu_fwd_bf16(x.data_ptr(), -1, y.data_ptr(), s) == L.EINVAL
    assert lib.scn_relu_bwd_bf16(x.data_ptr(), x.data_ptr(), -1, y.data_ptr(), s) == L.EINVAL
    assert lib.scn_relu_fwd_bf16(0, 16, y.data_ptr(), s) == L.EINVAL and lib.scn_relu_fwd_bf16(x.data_ptr(), 16, 0, s) == L.EINVAL
    for a in ((0, x.data_ptr(), y.data_ptr()), (x.data_ptr(), 0, y.data_ptr()), (x.data_ptr(), x.data_ptr(), 0)):
        assert lib.scn_relu_bwd_bf16(a[0], a[1], 16, a[2], s) == L.EINVAL, a
    torch.cuda.synchronize()
    assert bool((y == 0x5A5A).all())


# ---- 2. functional.ReLUFunction --------------------------------------------------------------------------------------------------
def test_relufunction_dispatches_on_dtype(operands):
    from sparse_rcnn_amd import functional as F
    n, c = 4099, 24
    xb = operands[0][:n * c].view(torch.bfloat16).view(n, c).clone().requires_grad_()
    gb = operands[1][:n * c].view(torch.bfloat16).view(n, c)
    y = F.ReLUFunction.apply(xb)
    (dx,) = torch.autograd.grad(y, xb, gb)
    assert y.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16 and y.shape == xb.shape
    xw = _widen(xb.detach().view(torch.int16)).requires_grad_()
    yw = F.ReLUFunction.apply(xw)
    (dxw,) = torch.autograd.grad(yw, xw, _widen(gb.view(torch.int16)))
    assert yw.dtype == torch.float32
    assert torch.equal(y.detach().view(torch.int16), _narrow(yw.detach()))
    assert torch.equal(dx.view(torch.int16), _narrow(dxw))
    # fp32: the result it always gave
    f = torch.randn(n, c, generator=torch.Generator().manual_seed(5)).to(DEV).requires_grad_()
    gf = torch.randn(n, c, generator=torch.Generator().manual_seed(6)).to(DEV)
    yf = F.ReLUFunction.apply(f)
    (df,) = torch.autograd.grad(yf, f, gf)
    assert yf.dtype == torch.float32 and torch.equal(yf, torch.relu(f.detach()))
    assert torch.equal(df, torch.where(f.detach() > 0, gf, torch.zeros_like(gf)))


# ---- 3. MultiLevelRpn with the heads on bf16 level tensors against the fp32-tail twin --------------------------------------------
# tests/test_gpu_anchor_up.py's smallest workload: 12 crops of 64 x 32 x 32, 1864 inside anchors per crop
GRID, TARGET = (64, 32, 32), 3000


def _step(**kw):
    from sparse_rcnn_amd.trainstep import SceneStep
    return SceneStep("ref-crop-rpn", grid=GRID, target=TARGET, prefetch=False, **kw)


def _levels(st):
    m = st.model
    with torch.no_grad():
        m.backbone(st.coords, st.feats, st.size, st.batch_size, metadata=None)
    return [m.backbone.unet.interims[i] for i in m.rpn_levels]


def _leaves(lv):
    from sparse_rcnn_amd.tensor import SparseConvNetTensor
    return [SparseConvNetTensor(features=t.features.detach().clone().requires_grad_(), metadata=t.metadata,
                                spatial_size=t.spatial_size) for t in lv]


class _ReLUSpy:
    """Stands in for functional.ReLUFunction while a test watches it: records every input's dtype; `widen` makes it the twin's
    tail, x.float() followed by the fp32 function."""

    def __init__(self, real, widen):
        self.real, self.widen, self.seen = real, widen, []

    def apply(self, x):
        self.seen.append(x.dtype)
        return self.real.apply(x.float() if self.widen else x)


def test_heads_behind_a_bf16_stack_equal_the_fp32_tail_twin(monkeypatch):
    from sparse_rcnn_amd import functional as F
    from sparse_rcnn_amd import rpn as R
    st = _step(dtype="bf16")
    lv = _levels(st)
    assert all(t.features.dtype == torch.bfloat16 for t in lv)
    levels = [(st.channels[2], 4, 128, R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS[0]),
              (st.channels[3], 8, 256, R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS[1])]
    torch.manual_seed(12)
    rpn = R.MultiLevelRpn(levels, num_dilations=5, autocast_bf16=True, keep_volume=True,
                          extra_stride_levels=R.REF_EXTRA_STRIDE_LEVELS).to(DEV)
    heads = list(rpn.anchor_network.parameters())
    stacks = [p for l in rpn.levels for p in l.stack.parameters()]
    assert len(heads) == 22 and len(stacks) == 20

    def run(widen):
        spy = _ReLUSpy(F.ReLUFunction, widen)
        monkeypatch.setattr(F, "ReLUFunction", spy)
        leaves = _leaves(lv)
        bbox, score, anchors = rpn(leaves)
        monkeypatch.undo()
        kept = (rpn.volume, rpn.volume_stored, rpn.volume_stored)
        grads = torch.autograd.grad(score.sum() + bbox.square().sum(), heads + stacks + [t.features for t in leaves])
        return bbox.detach(), score.detach(), anchors, grads, kept, spy.seen

    bbox, score, anchors, grads, (vol, vs, vs_again), seen = run(False)
    tb, ts, ta, tgrads, (tvol, _, _), tseen = run(True)
    assert seen == [torch.bfloat16] * 2 and tseen == [torch.bfloat16] * 2            # one stand-alone ReLU per level, on the stored slab
    assert tuple(score.shape) == (st.batch_size, 1864)
    assert torch.equal(bbox, tb) and torch.equal(score, ts) and torch.equal(anchors, ta)
    names = [f"head {i}" for i in range(22)] + [f"stack {i}" for i in range(20)] + ["level 0 features", "level 1 features"]
    for name, a, b in zip(names, grads, tgrads):
        assert a.dtype == b.dtype and torch.equal(a, b), name
        assert bool(torch.isfinite(a.float()).all()), name
    assert grads[-1].dtype == torch.bfloat16 and float(grads[-1].float().abs().sum()) > 0
    # the kept volume: the stored form IS the bf16 ReLU's output -- no cast launched for it -- and widens to `volume` exactly
    assert vs[0].dtype == torch.bfloat16 and vol[0].dtype == torch.float32 and vs is vs_again
    assert type(vs[0].grad_fn).__name__ == "ReLUFunctionBackward"
    assert vol[0].grad_fn.next_functions[0][0] is vs[0].grad_fn                        # volume = that tensor .float()
    assert torch.equal(vs[0].detach().float(), vol[0].detach())
    assert torch.equal(tvol[0].detach(), vol[0].detach())                             # the twin kept the same values
    st.finish()


# ---- 4. the step -----------------------------------------------------------------------------------------------------------------
ALL_LOSSES = dict(dtype="bf16", upsample_heads=True, rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True,
                  optimizer="adam", n_gt=8)


def _one_step(**kw):
    st = _step(**kw)
    d = st.describe()
    up = st.model.rpn.anchor_network
    assert up is not None and all(l.head is None and l.autocast_bf16 for l in st.model.rpn.levels)
    st.step()
    losses = [float(v.detach().cpu()) for v in (*st.rpn_losses, st.mask_losses, st.class_losses, st.segmentation_losses)]
    print("[relu bf16 step] losses (rpn score, rpn bbox, mask, class, segmentation):", " ".join(f"{v:.5f}" for v in losses))
    assert len(losses) == 5 and np.isfinite(losses).all()
    assert tuple(st.rpn_out[1].shape) == (st.batch_size, 1864) and st.rpn_out[1].dtype == torch.float32
    for h in up.heads():
        for p in (h.weight, h.bias):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    out = st.predict()
    st.finish()
    assert {"roi_bbox", "class", "mask", "segmentation_class"} <= set(out)
    return d, losses, st.flat.flat.detach().clone(), torch.cat([b.reshape(-1) for b in out["roi_bbox"]]).clone()


def test_scenestep_bf16_with_the_heads_and_a_bf16_class_branch():
    runs = [_one_step(dense_class=True, class_storage="bf16", **ALL_LOSSES) for _ in range(2)]
    d = runs[0][0]
    assert "AnchorNetworkUpsample heads" in d and "1x1 head" not in d
    assert "scn_relu_fwd_bf16" in d and "bf16-STORED stack" in d and "class_storage bf16" in d
    assert runs[0][1] == runs[1][1]                                          # two equally seeded runs: the same bits
    assert bool(torch.isfinite(runs[0][2]).all())
    assert torch.equal(runs[0][2], runs[1][2]) and torch.equal(runs[0][3], runs[1][3])


@pytest.mark.parametrize("kw, stack_bf16", [(dict(dense_class=True), True), (dict(), True), (dict(dtype="bf16-blocks"), False)],
                         ids=["fp32-dense-class-branch", "sparse-class-branch", "bf16-blocks"])
def test_scenestep_bf16_with_the_heads_other_class_branches(kw, stack_bf16):
    """Without class_storage, without dense_class, and on bf16-blocks storage (the units' slabs only: the RPN's level tensors
    and with them its stacks are fp32 there, and describe() does not name the bf16 ReLU)."""
    d, losses, flat, _ = _one_step(**{**ALL_LOSSES, **kw})
    assert ("scn_relu_fwd_bf16" in d) == stack_bf16 and "class_storage bf16" not in d
    assert bool(torch.isfinite(flat).all())


# ---- 5. unchanged defaults -------------------------------------------------------------------------------------------------------
def test_the_1x1_heads_on_bf16_storage_launch_what_they_launched(monkeypatch):
    """SceneStep('ref-crop-rpn', dtype='bf16', rpn_loss=True): its MultiLevelRpn is the composition of DenseRpn levels with the
    same parameters, bit for bit, and its stand-alone ReLUs still run in fp32 on the widened slab."""
    from sparse_rcnn_amd import functional as F
    from sparse_rcnn_amd import rpn as R
    st = _step(dtype="bf16", rpn_loss=True)
    mine = st.model.rpn
    assert mine.anchor_network is None and "1x1 head" in st.describe() and "scn_relu_fwd_bf16" not in st.describe()
    lv = _levels(st)
    levels = [(st.channels[2], 4, 128, R.REF_ANCHOR_LEVELS_VOXELS[0]), (st.channels[3], 8, 256, R.REF_ANCHOR_LEVELS_VOXELS[1])]
    hand = torch.nn.ModuleList(R.DenseRpn(c, stride, width, 5, tuple(map(tuple, a)), True, None, keep_inside=False,
                                          keep_volume=False) for c, stride, width, a in levels).to(DEV)
    hand.load_state_dict(mine.levels.state_dict())
    spy = _ReLUSpy(F.ReLUFunction, False)
    monkeypatch.setattr(F, "ReLUFunction", spy)
    with torch.no_grad():
        bbox, score, anchors = mine(lv)
        n_mine = len(spy.seen)
        outs = [r(t) for r, t in zip(hand, lv)]
    monkeypatch.undo()
    assert n_mine == 2 and spy.seen == [torch.float32] * 4
    all_anchors = torch.cat([o[2] for o in outs], 0)
    idx = R.inside_indicator(all_anchors, torch.tensor(GRID, dtype=torch.float32)).nonzero().squeeze(1)
    assert idx.numel() > 0
    assert torch.equal(bbox, torch.cat([o[0] for o in outs], 1).index_select(1, idx))
    assert torch.equal(score, torch.cat([o[1] for o in outs], 1).index_select(1, idx))
    assert torch.equal(anchors, all_anchors[idx])
    st.finish()
    from sparse_rcnn_amd.trainstep import SceneStep
    with pytest.raises(ValueError, match="ref-crop-rpn"):
        SceneStep("cfg3-rpn", upsample_heads=True)
