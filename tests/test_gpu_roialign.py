"""MI355X: the dense RoiAlign (scn_roialign_fwd / _bwd), the unclamped dense max pool (scn_dense_maxpool_fwd / _bwd), their
Python surface (functional.RoiAlignFunction / DenseMaxPoolFunction, roi.transform_boxes_interpolation, roi.RoiAlign),
classhead.DenseClassBranch and the step that uses it, against the fixtures the reference's own code produced
(tests/golden/make_roialign_golden.py) and the restatement (tests/roialign_restate.py).

Bars (tests/test_roialign_cpu.py derives them): bbox_tensor bit-equal; output max|got - ref| <= 2e-6 max|F|; gradients relative
L2 <= 2e-5; the max pool bit-equal to torch's max_pool3d in both directions; class scores within 1e-4 of the score scale."""
import json
import os

import numpy as np
import pytest
import torch

import roialign_restate as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
CASES = ["mixed", "small8", "aniso", "whole40", "empty"]
OUT_BAR, GRAD_BAR = 2e-6, 2e-5
DEV = "cuda"


def _case(name):
    return R.load_case(os.path.join(GOLDEN, f"roialign_{name}.npz"))


@pytest.mark.parametrize("name", CASES)
def test_transform_boxes_interpolation(name):
    from sparse_rcnn_amd import roi
    z = _case(name)
    boxes = [torch.from_numpy(b) for b in z["bbox_batch"]]
    bbox, counts, assoc = roi.transform_boxes_interpolation(boxes, z["_size"], True, z["_stride"])
    assert bbox.is_cuda and bbox.dtype == torch.float32 and tuple(bbox.shape) == tuple(z["bbox_tensor"].shape)
    assert bbox.cpu().numpy().tobytes() == z["bbox_tensor"].tobytes()
    assert counts == [int(v) for v in z["counts"]]
    assert assoc.tolist() == [s for s, c in enumerate(counts) for _ in range(c)]


def _with_canaries(rows, c, value=777.0):
    """A [rows, c] view in the middle of a buffer with 8 canary rows on either side."""
    buf = torch.full((rows + 16, c), value, dtype=torch.float32, device=DEV)
    return buf, buf[8:8 + rows]


def _raw_forward_backward(z):
    """The two entry points on canaried buffers -> (Out, dF of run 1, dF of run 2, canaries intact)."""
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.functional import _host3
    lib = L.lib()
    c, size, extract, batch = z["_c"], z["_size"], z["_extract"], z["_batch"]
    r = z["bbox_tensor"].shape[0]
    vol = torch.from_numpy(z["volume"]).to(DEV).reshape(-1, c)
    boxes = torch.from_numpy(z["bbox_tensor"]).to(DEV)
    sample = torch.tensor([s for s, n in enumerate(z["counts"]) for _ in range(int(n))], dtype=torch.int32, device=DEV)
    n_out = r * extract[0] * extract[1] * extract[2]
    obuf, out = _with_canaries(n_out, c)
    table = torch.empty(max(r, 1) * (3 * sum(extract) + 2 * sum(size)), dtype=torch.int32, device=DEV)   # include/scn_mi355x.h
    L.check(lib.scn_roialign_fwd(L.ptr(vol), batch, _host3(size), c, L.ptr(boxes), L.ptr(sample), r, _host3(extract),
                                 L.ptr(table), L.ptr(out), L.stream()))
    dout = torch.from_numpy(z["dout"]).to(DEV).reshape(-1, c)
    grads, bufs = [], [obuf]
    for _ in range(2):
        gbuf, dF = _with_canaries(vol.shape[0], c)
        L.check(lib.scn_roialign_bwd(L.ptr(dout), L.ptr(table), L.ptr(sample), r, batch, _host3(size), c, _host3(extract),
                                     L.ptr(dF), L.stream()))
        grads.append(dF)
        bufs.append(gbuf)
    torch.cuda.synchronize()
    intact = all(bool((b[:8] == 777.0).all()) and bool((b[-8:] == 777.0).all()) for b in bufs)
    return out, grads[0], grads[1], intact


@pytest.mark.parametrize("name", CASES)
def test_roialign_forward_against_the_fixture(name):
    z = _case(name)
    out, _, _, intact = _raw_forward_backward(z)
    assert intact
    rows = out.cpu().numpy()
    if rows.shape[0] == 0:
        assert z["out_rows"].shape[0] == 0
        return
    err = np.abs(rows[::int(z["out_step"])] - z["out_rows"]).max() / float(z["vol_absmax"])
    print(f"[roialign fwd] {name}: max|got - ref| / max|F| = {err:.2e}")
    assert err <= OUT_BAR
    assert abs(np.sqrt((rows.astype(np.float64) ** 2).sum()) - float(z["out_norm"])) <= 1e-5 * float(z["out_norm"])


@pytest.mark.parametrize("name", CASES)
def test_roialign_backward_against_the_fixture(name):
    z = _case(name)
    _, g1, g2, intact = _raw_forward_backward(z)
    assert intact                                                   # canary rows before and after dF and Out
    assert torch.equal(g1, g2)                                      # deterministic: two runs, the same bits
    grad = g1.cpu().numpy()
    zero = np.unpackbits(z["grad_zero_rows"])[:grad.shape[0]].astype(bool)
    assert (grad[zero] == 0).all()                                  # cells no sample touches: exactly 0
    cells = z["_size"][0] * z["_size"][1] * z["_size"][2]
    for s, n in enumerate(z["counts"]):
        if int(n) == 0:
            assert (grad[s * cells:(s + 1) * cells] == 0).all()     # a sample without a box
    if z["bbox_tensor"].shape[0] == 0:
        assert (grad == 0).all()
        return
    rel = R.rel_l2(grad[::int(z["grad_step"])], z["grad_rows"])
    print(f"[roialign bwd] {name}: relative L2 {rel:.2e} (the reference's own fp32 vs fp64: {float(z['ref_grad_rel_l2']):.2e})")
    assert rel <= GRAD_BAR
    assert abs(np.sqrt((grad.astype(np.float64) ** 2).sum()) - float(z["grad_norm"])) <= 1e-4 * float(z["grad_norm"])


@pytest.mark.parametrize("c", [1, 12, 32, 40])
def test_channel_counts_against_the_restatement(c):
    """Case small8's geometry at other widths: the scalar form (1), the 16-byte form with a partial wave (12, 40), and 32."""
    from sparse_rcnn_amd.functional import RoiAlignFunction
    z = _case("small8")
    vol = torch.from_numpy(R.seeded_volume(40 + c, z["_batch"], z["_size"], c)).to(DEV)
    boxes = torch.from_numpy(z["bbox_tensor"]).to(DEV)
    sample = torch.tensor([s for s, n in enumerate(z["counts"]) for _ in range(int(n))], dtype=torch.int32, device=DEV)
    dout = torch.from_numpy(R.seeded_dout(40 + c, boxes.shape[0], z["_extract"], c)).to(DEV)
    a = vol.reshape(-1, c).clone().requires_grad_()
    out = RoiAlignFunction.apply(a, boxes, sample, z["_batch"], z["_size"], z["_extract"])
    out.backward(dout.reshape(-1, c))
    b = vol.clone().requires_grad_()
    ref = R.roialign(b, boxes, sample.long(), z["_extract"])
    ref.backward(dout)
    err = float((out.detach().view_as(ref) - ref.detach()).abs().max() / vol.abs().max())
    rel = R.rel_l2(a.grad.cpu().numpy(), b.grad.reshape(-1, c).cpu().numpy())
    print(f"[roialign C={c}] out {err:.2e} grad rel L2 {rel:.2e}")
    assert err <= OUT_BAR and rel <= GRAD_BAR


def _pool_inputs():
    g = torch.Generator().manual_seed(3)
    x = torch.randn((3, 4, 6, 2, 5), generator=g)                              # [R, ex, ey, ez, C], odd C: the scalar form
    ties = torch.randn((2, 4, 4, 4, 8), generator=g)
    ties[0, :2, :2, :2] = 0.25                                                  # an all-equal block
    ties[0, 2:, 2:, 2:, :4] = -1.5
    ties[1, 0, 0, 1] = ties[1, 0, 0, 0] = ties[1].max() + 1.0                   # pairwise ties of the maximum
    ties[1, 3, 2, 3] = ties[1, 2, 3, 2] = ties[1].max() + 2.0
    neg = -torch.rand((2, 2, 4, 4, 12), generator=g) - 0.5                       # all negative: a clamp at 0 would show
    return {"random": x, "ties": ties, "negative": neg}


@pytest.mark.parametrize("kind", ["random", "ties", "negative"])
def test_dense_max_pool_bit_equal_to_torch(kind):
    from sparse_rcnn_amd.functional import DenseMaxPoolFunction
    x = _pool_inputs()[kind]
    r, extent, c = x.shape[0], tuple(x.shape[1:4]), x.shape[4]
    ref_in = x.permute(0, 4, 1, 2, 3).contiguous().requires_grad_()
    ref = torch.nn.functional.max_pool3d(ref_in, 2)
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(4))
    ref.backward(g)
    a = x.reshape(-1, c).to(DEV).requires_grad_()
    y = DenseMaxPoolFunction.apply(a, r, extent)
    y.backward(g.permute(0, 2, 3, 4, 1).reshape(-1, c).to(DEV))
    assert torch.equal(y.detach().cpu().view(r, extent[0] // 2, extent[1] // 2, extent[2] // 2, c), ref.detach().permute(0, 2, 3, 4, 1))
    assert torch.equal(a.grad.cpu().view(x.shape), ref_in.grad.permute(0, 2, 3, 4, 1))
    if kind == "negative":
        assert bool((y < 0).all())
    # the padded form: rows of the padding boxes are zero, the gradient of the real rows is the same
    a2 = x.reshape(-1, c).to(DEV).requires_grad_()
    y2 = DenseMaxPoolFunction.apply(a2, r, extent, r + 3)
    assert y2.shape[0] == (r + 3) * y.shape[0] // r and torch.equal(y2[:y.shape[0]], y) and bool((y2[y.shape[0]:] == 0).all())


def test_roi_align_module():
    from sparse_rcnn_amd import roi
    z = _case("small8")
    c = z["_c"]
    boxes = [torch.from_numpy(b) for b in z["bbox_batch"]]
    with pytest.raises(NotImplementedError):
        roi.RoiAlign(z["_extract"], clip_boxes=False)
    with pytest.raises(NotImplementedError):
        roi.RoiAlign(z["_extract"], padding=0.0, clip_boxes=True)
    align = roi.RoiAlign(z["_extract"], clip_boxes=True, resize_boxes=z["_stride"])
    ncxyz = torch.from_numpy(z["volume"]).to(DEV).permute(0, 4, 1, 2, 3).contiguous()
    cl = ncxyz.contiguous(memory_format=torch.channels_last_3d)
    assert ncxyz.is_contiguous() and cl.is_contiguous(memory_format=torch.channels_last_3d)
    out_a, (bbox_a, counts_a, shape_a) = align(ncxyz, boxes)
    out_b, (bbox_b, counts_b, shape_b) = align(cl, boxes)
    r = bbox_a.shape[0]
    assert tuple(out_a.shape) == (r, c) + z["_extract"] and torch.equal(out_a, out_b)
    assert bbox_a.cpu().numpy().tobytes() == z["bbox_tensor"].tobytes() and torch.equal(bbox_a, bbox_b)
    assert counts_a == counts_b == [int(v) for v in z["counts"]] and tuple(shape_a) == tuple(shape_b) == z["_size"]
    rows = out_a.permute(0, 2, 3, 4, 1).reshape(-1, c).cpu().numpy()
    assert np.abs(rows[::int(z["out_step"])] - z["out_rows"]).max() <= OUT_BAR * float(z["vol_absmax"])
    empty, (bbox_e, counts_e, _) = align(cl, [b[:0] for b in boxes])
    assert tuple(empty.shape) == (0, c) + z["_extract"] and bbox_e.shape == (0, 2, 3) and counts_e == [0, 0]


def test_dense_class_branch_against_the_fixture():
    from sparse_rcnn_amd.classhead import DenseClassBranch, conv3d_to_slab_weight
    small = json.load(open(os.path.join(GOLDEN, "dense_class_small.json")))
    z = dict(np.load(os.path.join(GOLDEN, "dense_class_small.npz")))
    seed, batch, size, c = int(z["seed"]), int(z["batch"]), tuple(int(v) for v in z["size"]), int(z["c"])
    params = R.seeded_params(small["keys"], seed)
    branch = DenseClassBranch(12, 8, 8, (8, 16), (8,), 5).to(DEV)
    assert branch.load_reference_state_dict({k: torch.from_numpy(v) for k, v in params.items()}) == ([], [])
    vol = torch.from_numpy(R.seeded_volume(seed, batch, size, c)).to(DEV).reshape(-1, c).requires_grad_()
    counts, o, boxes = [int(v) for v in z["counts"]], 0, []
    for n in counts:
        boxes.append(torch.from_numpy(z["boxes"][o:o + n]).to(DEV))
        o += n
    scores, (bbox, got_counts, got_size) = branch(vol, size, batch, boxes)
    assert got_counts == counts and tuple(got_size) == size and bbox.cpu().numpy().tobytes() == z["bbox_tensor"].tobytes()
    scale = float(np.abs(z["scores"]).max())
    err = float(np.abs(scores.detach().cpu().numpy() - z["scores"]).max())
    print(f"[dense class] scores max err {err:.2e} (scale {scale:.3g})")
    assert err <= 1e-4 * scale
    n_md = len(branch._md)
    scores.backward(torch.from_numpy(z["score_grad"]).to(DEV))
    rel = R.rel_l2(vol.grad.cpu().numpy(), z["volume_grad"])
    print(f"[dense class] volume gradient rel L2 {rel:.2e}")
    assert rel <= GRAD_BAR
    step = int(z["element_step"])
    own = branch.named_oracle_params()
    for rk, name in branch.reference_key_map().items():
        g = own[name].grad.detach().cpu()
        ref = z["grad/" + rk]
        if g.dim() == 3:                                        # back to the reference's Conv3d layout
            k = round(g.shape[0] ** (1 / 3))
            from sparse_rcnn_amd.classhead import slab_to_conv3d_weight
            g = slab_to_conv3d_weight(g, k).contiguous()
        g = g.numpy().reshape(-1)
        rel = R.rel_l2(g if ref.size == g.size else g[::step], ref)
        print(f"[dense class] {rk}: gradient rel L2 {rel:.2e}")
        assert rel <= GRAD_BAR, rk
    # another R in the same bucket: no new Metadata; an R in another bucket: the same scores for the shared boxes
    with torch.no_grad():
        fewer, _ = branch(vol, size, batch, [boxes[0][:2], boxes[1]])
        assert len(branch._md) == n_md
        extra = torch.from_numpy(np.tile(z["boxes"][:1], (32, 1, 1))).to(DEV)
        more, (_, more_counts, _) = branch(vol, size, batch, [boxes[0], torch.cat([boxes[1], extra])])
    assert len(branch._md) == n_md + 1 and more_counts == [counts[0], counts[1] + 32]
    assert branch.bucket(sum(counts)) == 32 and branch.bucket(sum(counts) + 32) == 64
    ref_scores = scores.detach()
    assert float((more[:sum(counts)] - ref_scores).abs().max()) <= 1e-5 * scale
    keep = [0, 1] + list(range(counts[0], sum(counts)))
    assert float((fewer - ref_scores[keep]).abs().max()) <= 1e-5 * scale
    assert float((more[sum(counts):] - more[sum(counts):sum(counts) + 1]).abs().max()) == 0      # 32 copies of one box in sample 1


def test_scenestep_with_the_dense_class_branch():
    from sparse_rcnn_amd.classhead import ClassBranch, DenseClassBranch
    from sparse_rcnn_amd.trainstep import SceneStep
    kw = dict(optimizer='adam', rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True)
    st = SceneStep('cfg3-rpn', dense_class=True, **kw)
    assert isinstance(st.model.class_branch, DenseClassBranch) and "DENSE class branch" in st.describe()
    assert st._size_factor == 2 ** (len(st.channels) - 1)
    for _ in range(2):
        st.step()
        for loss in (*st.rpn_losses, st.mask_losses, st.class_losses, st.segmentation_losses):
            assert bool(torch.isfinite(loss))
    st.finish()
    assert st.class_out[0].shape[1] == 18 and st.class_out[0].shape[0] == torch.cat(st.class_out[3]).numel()
    # the gradient that enters at the class scores reaches `model.rpn.stack.0.weight`, the first convolution of the RPN's dilation
    # stack; on the sparse arm the class branch reads the encoder level and that parameter is not in its graph at all
    sparse = SceneStep('cfg3-rpn', **kw)
    assert isinstance(sparse.model.class_branch, ClassBranch)
    got = {}
    for name, step in (("dense", st), ("sparse", sparse)):
        m = step.model
        m.backbone(step.coords, step.feats, step.size, step.batch_size, metadata=None)
        interims = m.backbone.unet.interims
        m.run_rpn(interims)
        scores, _ = m.run_class(interims, [b.float().to(step.device) for b in step.gt_boxes])
        (got[name],) = torch.autograd.grad(scores.sum(), [dict(m.named_parameters())["rpn.stack.0.weight"]], allow_unused=True)
    assert got["sparse"] is None
    assert got["dense"] is not None and bool(torch.isfinite(got["dense"]).all()) and float(got["dense"].abs().sum()) > 0
    # predict() and evaluate() return what they return on the sparse arm
    out, ref = st.predict(), sparse.predict()
    st.finish()
    sparse.finish()
    assert set(out) == set(ref) and {"roi_bbox", "class", "class_propabilities", "mask", "segmentation_class"} <= set(out)
    n_kept = [int(b.shape[0]) for b in out["roi_bbox"]]
    assert sum(n_kept) > 0 and st.predict_out[0].shape == (sum(n_kept), 18)
    assert [tuple(c.shape) for c in out["class"]] == [(n,) for n in n_kept]
    combined, single = st.evaluate(score_threshold=0.5)
    ref_combined, ref_single = sparse.evaluate(score_threshold=0.5)
    assert set(combined) == set(ref_combined) and set(single) == set(ref_single)
    assert all(np.isfinite(v) or np.isnan(v) for v in combined.values())
