"""MI355X: bf16 storage in the dense class branch -- the bf16 entry points of the dense RoiAlign and of the unclamped dense max pool
(scn_roialign_fwd_bf16 / _bwd_bf16, scn_dense_maxpool_fwd_bf16 / _bwd_bf16), their Python surface, roi.RoiAlign on a bf16 map,
classhead.DenseClassBranch(storage=torch.bfloat16) and SceneStep(class_storage="bf16").

Notation: q = round to bf16, M = max|F|.  Bars:
  forward, elementwise against the float64 restatement on the bf16 inputs:  |got - ref| <= 2^-8 |ref| + 2.1e-6 M  (the fp32
      kernel's 2e-6 M bar against float64, tests/test_roialign_cpu.py, plus one rounding of the result);
  backward: relative L2 <= 2^-8 + 2e-5 (one rounding plus the fp32 gradient bar);
  both hold for the once-rounded fp32 restatement itself (tests/test_roialign_bf16_cpu.py: worst forward slack -3.9e-6, backward
      1.5e-3 .. 1.7e-3 over the twelve cases);
  every bf16 entry point against its fp32 twin on the widened inputs, rounded once: equal bits;
  max pool against torch's max_pool3d on the widened values: equal bits, both directions;
  the branch against the restatement with the same roundings (tests/dense_class_bf16_restate.py): scores within 2^-6 of the score
      scale, every gradient within 2e-2 relative L2 -- the project's bf16 bars (tests/test_gpu_atsize.py, FROZEN_L2_BF16)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import dense_class_bf16_restate as D
import roialign_restate as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
DEV = "cuda"
BF = torch.bfloat16
CANARY = 768.0                          # a bf16 value
FWD_BF16, FROZEN_L2_BF16 = 2.0 ** -6, 2e-2


@functools.lru_cache(maxsize=None)
def _case(name):
    return R.load_case(os.path.join(GOLDEN, f"roialign_{name}.npz"))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _with_canaries(rows, c, dtype=BF):
    """A [rows, c] view in the middle of a buffer with 8 canary rows on either side (8 rows of c >= 8 bf16: 16-byte aligned)."""
    buf = torch.full((rows + 16, c), CANARY, dtype=dtype, device=DEV)
    return buf, buf[8:8 + rows]


def _intact(bufs):
    return all(bool((b[:8] == CANARY).all()) and bool((b[-8:] == CANARY).all()) for b in bufs)


def _table(r, size, extract):
    return torch.empty(max(r, 1) * (3 * sum(extract) + 2 * sum(size)), dtype=torch.int32, device=DEV)     # include/scn_mi355x.h


def _raw(z, vol, boxes, sample, dout, bf16):
    """Forward and two backwards of the raw entry points on canaried buffers -> (Out, dF run 1, dF run 2, canaries intact)."""
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.functional import _host3
    lib = L.lib()
    fwd, bwd = (lib.scn_roialign_fwd_bf16, lib.scn_roialign_bwd_bf16) if bf16 else (lib.scn_roialign_fwd, lib.scn_roialign_bwd)
    dt = BF if bf16 else torch.float32
    c, size, extract, batch, r = vol.shape[-1], z["_size"], z["_extract"], z["_batch"], boxes.shape[0]
    vol, dout = vol.to(DEV, dt).reshape(-1, c).contiguous(), dout.to(DEV, dt).reshape(-1, c).contiguous()
    boxes, sample = boxes.to(DEV), sample.to(DEV, torch.int32)
    obuf, out = _with_canaries(r * extract[0] * extract[1] * extract[2], c, dt)
    table = _table(r, size, extract)
    L.check(fwd(L.ptr(vol), batch, _host3(size), c, L.ptr(boxes), L.ptr(sample), r, _host3(extract), L.ptr(table), L.ptr(out),
                L.stream()))
    grads, bufs = [], [obuf]
    for _ in range(2):
        gbuf, dF = _with_canaries(vol.shape[0], c, dt)
        L.check(bwd(L.ptr(dout), L.ptr(table), L.ptr(sample), r, batch, _host3(size), c, _host3(extract), L.ptr(dF), L.stream()))
        grads.append(dF)
        bufs.append(gbuf)
    torch.cuda.synchronize()
    return out, grads[0], grads[1], _intact(bufs)


@functools.lru_cache(maxsize=None)
def _raw_bf16(name, c):
    z = _case(name)
    return _raw(z, *D.bf16_case(z, c), bf16=True)


# ---- 1. the raw entry points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", D.WIDTHS)
@pytest.mark.parametrize("name", D.GEOMETRIES)
def test_forward_against_the_float64_restatement(name, c):
    z = _case(name)
    out, _, _, intact = _raw_bf16(name, c)
    assert intact and out.dtype == BF
    ref, _ = D.float64_reference(name, z, c)
    absmax = float(D.bf16_case(z, c)[0].abs().max())
    slack = D.forward_slack(out.float().cpu().view_as(ref), ref, absmax)
    print(f"[roialign bf16 fwd] {name} C={c}: worst |got - ref| - (2^-8 |ref| + 2.1e-6 M) = {slack:.2e}")
    assert slack <= 0


@pytest.mark.parametrize("c", D.WIDTHS)
@pytest.mark.parametrize("name", D.GEOMETRIES)
def test_backward_against_the_float64_restatement(name, c):
    z = _case(name)
    _, g1, g2, intact = _raw_bf16(name, c)
    assert intact and g1.dtype == BF
    assert torch.equal(_bits(g1), _bits(g2))                           # two runs, the same bits
    grad = g1.float().cpu().numpy()
    zero = np.unpackbits(z["grad_zero_rows"])[:grad.shape[0]].astype(bool)
    assert (_bits(g1).cpu().numpy()[zero] == 0).all()                  # cells no sample touches: +0, every bit
    cells = z["_size"][0] * z["_size"][1] * z["_size"][2]
    for s, n in enumerate(z["counts"]):
        if int(n) == 0:
            assert (_bits(g1).cpu().numpy()[s * cells:(s + 1) * cells] == 0).all()     # a sample without a box
    _, ref = D.float64_reference(name, z, c)
    rel = D.rel_l2(grad, ref.reshape(-1, c).numpy())
    print(f"[roialign bf16 bwd] {name} C={c}: relative L2 {rel:.2e} (bar {D.GRAD_BAR:.2e})")
    assert rel <= D.GRAD_BAR


def test_no_boxes():
    """R = 0: the forward launches nothing (Out untouched), the backward writes an all-zero dF."""
    z = _case("empty")
    c = 8
    vol = D.bf16_round(torch.from_numpy(R.seeded_volume(48, z["_batch"], z["_size"], c)))
    out, g1, g2, intact = _raw(z, vol, torch.zeros((0, 2, 3)), torch.zeros(0, dtype=torch.long),
                               torch.zeros((0,) + z["_extract"] + (c,)), bf16=True)
    assert intact and out.shape[0] == 0
    assert g1.shape[0] == vol.numel() // c and bool((_bits(g1) == 0).all()) and bool((_bits(g2) == 0).all())


# ---- 2. bf16 entry point == fp32 entry point on the widened inputs, rounded once -----------------------------------------------
def test_bf16_equals_the_fp32_twin_rounded_once():
    z = _case("small8")
    vol, boxes, sample, dout = D.bf16_case(z, 32)
    out_h, grad_h, _, ok_h = _raw(z, vol, boxes, sample, dout, bf16=True)
    out_f, grad_f, _, ok_f = _raw(z, vol, boxes, sample, dout, bf16=False)          # the same values, widened exactly
    assert ok_h and ok_f and out_f.dtype == torch.float32
    assert torch.equal(_bits(out_h), _bits(out_f.to(BF)))
    assert torch.equal(_bits(grad_h), _bits(grad_f.to(BF)))
    assert not torch.equal(out_f, out_f.to(BF).float())                             # (the rounding is not vacuous)


# ---- 3. max pool -----------------------------------------------------------------------------------------------------------------
def _pool_input(kind, c):
    g = torch.Generator().manual_seed(3 + c)
    if kind == "random":
        x = torch.randn((3, 4, 6, 2, c), generator=g)
    elif kind == "ties":
        x = torch.randn((2, 4, 4, 4, c), generator=g)
        x[0, :2, :2, :2] = 0.25                                                  # an all-equal block
        x[0, 2:, 2:, 2:, :4] = -1.5
        x[1, 0, 0, 1] = x[1, 0, 0, 0] = x[1].max() + 1.0                         # pairwise ties of the maximum
        x[1, 3, 2, 3] = x[1, 2, 3, 2] = x[1].max() + 2.0
    else:
        x = -torch.rand((2, 2, 4, 4, c), generator=g) - 0.5                     # all negative: a clamp at 0 would show
    return D.bf16_round(x)                                                       # (rounding keeps ties tied and signs)


@pytest.mark.parametrize("c", [8, 16, 24])
@pytest.mark.parametrize("kind", ["random", "ties", "negative"])
def test_dense_max_pool_bit_equal_to_torch(kind, c):
    from sparse_rcnn_amd.functional import DenseMaxPoolFunction
    x = _pool_input(kind, c)
    r, extent = x.shape[0], tuple(x.shape[1:4])
    ref_in = x.permute(0, 4, 1, 2, 3).contiguous().requires_grad_()
    ref = torch.nn.functional.max_pool3d(ref_in, 2)
    g = D.bf16_round(torch.randn(ref.shape, generator=torch.Generator().manual_seed(4)))
    ref.backward(g)
    a = x.reshape(-1, c).to(DEV, BF).requires_grad_()
    y = DenseMaxPoolFunction.apply(a, r, extent)
    assert y.dtype == BF
    y.backward(g.permute(0, 2, 3, 4, 1).reshape(-1, c).to(DEV, BF))
    assert a.grad.dtype == BF
    got = y.detach().float().cpu().view(r, extent[0] // 2, extent[1] // 2, extent[2] // 2, c)
    assert torch.equal(got, ref.detach().permute(0, 2, 3, 4, 1))
    assert torch.equal(a.grad.float().cpu().view(x.shape), ref_in.grad.permute(0, 2, 3, 4, 1))
    if kind == "negative":
        assert bool((y.float() < 0).all())
    a2 = x.reshape(-1, c).to(DEV, BF).requires_grad_()
    y2 = DenseMaxPoolFunction.apply(a2, r, extent, r + 3)                        # the padded form
    assert y2.dtype == BF and y2.shape[0] == (r + 3) * y.shape[0] // r
    assert torch.equal(_bits(y2[:y.shape[0]]), _bits(y.detach())) and bool((_bits(y2[y.shape[0]:]) == 0).all())


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_widths_without_lanes_are_refused():
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.functional import DenseMaxPoolFunction, RoiAlignFunction, _host3
    z = _case("small8")
    boxes = torch.from_numpy(z["bbox_tensor"]).to(DEV)
    sample = torch.tensor([s for s, n in enumerate(z["counts"]) for _ in range(int(n))], dtype=torch.int32, device=DEV)
    cells = z["_batch"] * z["_size"][0] * z["_size"][1] * z["_size"][2]
    slab = torch.zeros((cells, 12), dtype=BF, device=DEV)
    with pytest.raises(ValueError, match="multiple of 8"):
        RoiAlignFunction.apply(slab, boxes, sample, z["_batch"], z["_size"], z["_extract"])
    with pytest.raises(ValueError, match="multiple of 8"):
        DenseMaxPoolFunction.apply(torch.zeros((2 * 64, 12), dtype=BF, device=DEV), 2, (4, 4, 4))
    lib, r = L.lib(), boxes.shape[0]
    out = torch.full((r * 512, 12), CANARY, dtype=BF, device=DEV)
    table = _table(r, z["_size"], z["_extract"])
    rc = lib.scn_roialign_fwd_bf16(L.ptr(slab), z["_batch"], _host3(z["_size"]), 12, L.ptr(boxes), L.ptr(sample), r,
                                   _host3(z["_extract"]), L.ptr(table), L.ptr(out), L.stream())
    assert rc == L.EINVAL and b"c % 8" in lib.scn_last_error_string()
    assert lib.scn_roialign_bwd_bf16(L.ptr(out), L.ptr(table), L.ptr(sample), r, z["_batch"], _host3(z["_size"]), 12,
                                     _host3(z["_extract"]), L.ptr(slab), L.stream()) == L.EINVAL
    arg = torch.zeros((r * 64, 12), dtype=torch.uint8, device=DEV)
    assert lib.scn_dense_maxpool_fwd_bf16(L.ptr(out), r, _host3(z["_extract"]), 12, L.ptr(slab), L.ptr(arg), L.stream()) == L.EINVAL
    assert lib.scn_dense_maxpool_bwd_bf16(L.ptr(slab), L.ptr(arg), r, _host3(z["_extract"]), 12, L.ptr(out), L.stream()) == L.EINVAL
    # a width with lanes at a pointer without 16-byte alignment
    odd = torch.zeros(cells * 8 + 8, dtype=BF, device=DEV)[1:]
    assert lib.scn_roialign_fwd_bf16(L.ptr(odd), z["_batch"], _host3(z["_size"]), 8, L.ptr(boxes), L.ptr(sample), r,
                                     _host3(z["_extract"]), L.ptr(table), L.ptr(out), L.stream()) == L.EINVAL
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())                                           # nothing was launched


# ---- 5. the module ---------------------------------------------------------------------------------------------------------------
def test_roi_align_module_on_a_bf16_map():
    from sparse_rcnn_amd import roi
    z = _case("small8")
    c = 8
    vol, _, _, _ = D.bf16_case(z, c)
    boxes = [torch.from_numpy(b) for b in z["bbox_batch"]]
    align = roi.RoiAlign(z["_extract"], clip_boxes=True, resize_boxes=z["_stride"])
    ncxyz = vol.to(DEV, BF).permute(0, 4, 1, 2, 3).contiguous()
    out, (bbox, counts, shape) = align(ncxyz, boxes)
    r = bbox.shape[0]
    assert out.dtype == BF and tuple(out.shape) == (r, c) + z["_extract"]
    assert bbox.dtype == torch.float32 and bbox.cpu().numpy().tobytes() == z["bbox_tensor"].tobytes()
    assert counts == [int(v) for v in z["counts"]] and tuple(shape) == z["_size"]
    raw, _, _, _ = _raw_bf16("small8", c)
    assert torch.equal(_bits(out.permute(0, 2, 3, 4, 1).reshape(-1, c)), _bits(raw))
    empty, (bbox_e, counts_e, _) = align(ncxyz, [b[:0] for b in boxes])
    assert empty.dtype == BF and tuple(empty.shape) == (0, c) + z["_extract"] and bbox_e.shape == (0, 2, 3) and counts_e == [0, 0]


# ---- 6. the branch ---------------------------------------------------------------------------------------------------------------
def test_dense_class_branch_bf16_against_the_restatement():
    from sparse_rcnn_amd import functional as F
    from sparse_rcnn_amd.classhead import DenseClassBranch, slab_to_conv3d_weight
    small = json.load(open(os.path.join(GOLDEN, "dense_class_small.json")))
    z = dict(np.load(os.path.join(GOLDEN, "dense_class_small.npz")))
    seed, batch, size, c = int(z["seed"]), int(z["batch"]), tuple(int(v) for v in z["size"]), 16
    shapes = dict(small["keys"])
    shapes["input_conv_layer.0.0.0.weight"] = [8, c, 1, 1, 1]                    # the fixture's network at 16 input channels
    params = {k: torch.from_numpy(v) for k, v in R.seeded_params(shapes, seed).items()}
    branch = DenseClassBranch(c, 8, 8, (8, 16), (8,), 5, storage=BF).to(DEV)
    assert branch.load_reference_state_dict(params) == ([], [])
    assert all(p.dtype == torch.float32 for p in branch.parameters())
    vol_cpu = D.bf16_round(torch.from_numpy(R.seeded_volume(seed, batch, size, c)))
    vol = vol_cpu.to(DEV, BF).reshape(-1, c).requires_grad_()
    counts, o, boxes = [int(v) for v in z["counts"]], 0, []
    for n in counts:
        boxes.append(torch.from_numpy(z["boxes"][o:o + n]))
        o += n
    seen = []
    hook = branch.output_conv_layer.register_forward_pre_hook(lambda m, args: seen.append(args[0].features.dtype))
    F.RELU_RECORD = []
    try:
        scores, (bbox, got_counts, got_size) = branch(vol, size, batch, [b.to(DEV) for b in boxes])
        masks = F.RELU_RECORD
    finally:
        F.RELU_RECORD = None
        hook.remove()
    assert seen == [BF]                                                          # the pooled slab is bf16-stored
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (sum(counts), 5)
    assert got_counts == counts and tuple(got_size) == size and bbox.cpu().numpy().tobytes() == z["bbox_tensor"].tobytes()
    assert len(masks) == 8                                                       # 3 units x 2 and the two ReLUs of the linear stack
    score_grad = torch.from_numpy(z["score_grad"])
    scores.backward(score_grad.to(DEV))
    assert vol.grad.dtype == BF

    sd = {k: v.clone().requires_grad_() for k, v in params.items()}
    ref_vol = vol_cpu.clone().requires_grad_()
    ref, ref_bbox, _ = D.dense_class_forward(sd, ref_vol.permute(0, 4, 1, 2, 3), boxes, float(z["stride"]), branch.cut_shape,
                                             q=D.bf16_round, wq=D.bf16_round, relu=D.FrozenMasks(masks))
    ref.backward(score_grad)
    assert ref_bbox.numpy().tobytes() == z["bbox_tensor"].tobytes()
    scale = float(ref.detach().abs().max())
    err = float((scores.detach().cpu() - ref.detach()).abs().max())
    print(f"[dense class bf16] scores max err {err:.2e} = {err / scale:.2e} of the scale {scale:.3g} (bar {FWD_BF16:.2e})")
    assert err <= FWD_BF16 * scale
    rel = D.rel_l2(vol.grad.float().cpu().numpy(), ref_vol.grad.reshape(-1, c).numpy())
    print(f"[dense class bf16] volume gradient rel L2 {rel:.2e}")
    assert rel <= FROZEN_L2_BF16
    own = branch.named_oracle_params()
    for rk, name in branch.reference_key_map().items():
        g = own[name].grad.detach().cpu()
        assert g.dtype == torch.float32
        if g.dim() == 3:                                                         # back to the reference's Conv3d layout
            g = slab_to_conv3d_weight(g, round(g.shape[0] ** (1 / 3))).contiguous()
        elif g.dim() == 2 and rk.startswith("linear_layer"):
            g = g.reshape(sd[rk].shape)
        rel = D.rel_l2(g.numpy().reshape(-1), sd[rk].grad.numpy().reshape(-1))
        print(f"[dense class bf16] {rk}: gradient rel L2 {rel:.2e}")
        assert rel <= FROZEN_L2_BF16, rk


# ---- 7. the step -----------------------------------------------------------------------------------------------------------------
def test_scenestep_with_class_storage_bf16():
    from sparse_rcnn_amd.trainstep import SceneStep
    kw = dict(optimizer='adam', rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True)
    with pytest.raises(ValueError):
        SceneStep('cfg3-rpn', dtype='f32', dense_class=True, class_storage='bf16', **kw)
    with pytest.raises(ValueError):
        SceneStep('cfg3-rpn', dtype='bf16', class_storage='bf16', **kw)
    st = SceneStep('cfg3-rpn', dtype='bf16', dense_class=True, class_storage='bf16', **kw)
    assert st.model.class_branch.storage is BF
    assert "bf16-STORED" in st.describe() and "scn_roialign_fwd_bf16" in st.describe()
    for _ in range(2):
        st.step()
        for loss in (*st.rpn_losses, st.mask_losses, st.class_losses, st.segmentation_losses):
            assert bool(torch.isfinite(loss))
    st.finish()
    stored = st.model.rpn.volume_stored
    assert stored[0].dtype == BF and torch.equal(stored[0].float(), st.model.rpn.volume[0]) and stored[1:] == st.model.rpn.volume[1:]
    plain = SceneStep('cfg3-rpn', dtype='bf16', dense_class=True, **kw)
    assert plain.model.class_branch.storage is torch.float32 and plain.class_storage is None
    assert "bf16-STORED" not in plain.describe()
    assert [n for n, _ in plain.model.named_parameters()] == [n for n, _ in st.model.named_parameters()]
    out, ref = st.predict(), plain.predict()
    st.finish()
    plain.finish()
    assert set(out) == set(ref) and {"roi_bbox", "class", "class_propabilities", "mask", "segmentation_class"} <= set(out)
