"""MI355X: RoiAlign + max pool in one pass (scn_roialign_pool_fwd / _bwd and their _bf16 forms), the box flatten
(scn_box_flatten_fwd / _bwd), their Python surface (functional.RoiAlignPoolFunction / BoxFlattenFunction),
classhead.ReshapeClassBranch, DenseClassBranch(fused_pool=True) and SceneStep(dense_class=True, simple_class=True).

Oracles.  The fused kernels: the library's own two-call chain (scn_roialign_fwd + scn_dense_maxpool_fwd;
scn_dense_maxpool_bwd + scn_roialign_bwd), which tests/test_gpu_roialign*.py hold against the reference -- forward Y and argmax
BIT-equal, backward equal as numbers (torch.equal: -0 == +0).  The flatten: the torch expression, bit-equal.  The branch: the
fixtures the reference's own ClassNetwork produced (tests/golden/make_reshape_class_golden.py) at the bars of
test_dense_class_branch_against_the_fixture: scores within 1e-4 of their scale, gradients within 2e-5 relative L2 (the
reference's own fp32 gradients are within 8e-7 of its float64 run)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import reshape_class_restate as S
import roialign_restate as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
DEV = "cuda"
BF = torch.bfloat16
CANARY = 768.0                          # (a bf16 value)
GEOMETRIES = ["mixed", "small8", "whole40", "empty", "aniso"]
SCORE_BAR, GRAD_BAR = 1e-4, 2e-5


@functools.lru_cache(maxsize=None)
def _case(name):
    return R.load_case(os.path.join(GOLDEN, f"roialign_{name}.npz"))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _canaried(rows, c, dtype, value=CANARY):
    """A [rows, c] view in the middle of a buffer with 8 canary rows on either side."""
    buf = torch.full((rows + 16, c), value, dtype=dtype, device=DEV)
    return buf, buf[8:8 + rows]


def _intact(bufs):
    return all(bool((b[:8] == CANARY).all()) and bool((b[-8:] == CANARY).all()) for b in bufs)


def _geometry(z):
    sample = torch.tensor([s for s, n in enumerate(z["counts"]) for _ in range(int(n))], dtype=torch.int32)
    return dict(size=z["_size"], extract=z["_extract"], batch=z["_batch"], boxes=torch.from_numpy(z["bbox_tensor"]), sample=sample)


def _both(geo, vol, dy, bf16):
    """The two-call chain and the fused calls on the same inputs -> dict of Y, arg, dF per side, the fused dF of a second run
    and whether the canary rows around the fused outputs are intact.  vol [B X Y Z, C], dy [R ex/2 ey/2 ez/2, C] (CPU fp32)."""
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.functional import _host3
    lib = L.lib()
    sfx = "_bf16" if bf16 else ""
    fn = {n: getattr(lib, f"scn_{n}{sfx}") for n in ("roialign_fwd", "roialign_bwd", "dense_maxpool_fwd", "dense_maxpool_bwd",
                                                     "roialign_pool_fwd", "roialign_pool_bwd")}
    dt = BF if bf16 else torch.float32
    size, extract, batch = geo["size"], geo["extract"], geo["batch"]
    boxes, sample = geo["boxes"].to(DEV), geo["sample"].to(DEV)
    r, c = boxes.shape[0], vol.shape[1]
    vol, dy = vol.to(DEV, dt).contiguous(), dy.to(DEV, dt).contiguous()
    n_out, cells = r * extract[0] * extract[1] * extract[2], vol.shape[0]
    hs, he = _host3(size), _host3(extract)
    table = lambda: torch.empty(max(r, 1) * (3 * sum(extract) + 2 * sum(size)), dtype=torch.int32, device=DEV)
    # the chain
    t0 = table()
    out = torch.empty((n_out, c), dtype=dt, device=DEV)
    y0 = torch.empty((n_out // 8, c), dtype=dt, device=DEV)
    a0 = torch.empty((n_out // 8, c), dtype=torch.uint8, device=DEV)
    L.check(fn["roialign_fwd"](L.ptr(vol), batch, hs, c, L.ptr(boxes), L.ptr(sample), r, he, L.ptr(t0), L.ptr(out), L.stream()))
    L.check(fn["dense_maxpool_fwd"](L.ptr(out), r, he, c, L.ptr(y0), L.ptr(a0), L.stream()))
    dout = torch.empty_like(out)
    df0 = torch.empty((cells, c), dtype=dt, device=DEV)
    L.check(fn["dense_maxpool_bwd"](L.ptr(dy), L.ptr(a0), r, he, c, L.ptr(dout), L.stream()))
    L.check(fn["roialign_bwd"](L.ptr(dout), L.ptr(t0), L.ptr(sample), r, batch, hs, c, he, L.ptr(df0), L.stream()))
    # fused, on canaried buffers and with a table of its own
    t1 = table()
    ybuf, y1 = _canaried(n_out // 8, c, dt)
    abuf, a1 = _canaried(n_out // 8, c, torch.uint8, 200)
    L.check(fn["roialign_pool_fwd"](L.ptr(vol), batch, hs, c, L.ptr(boxes), L.ptr(sample), r, he, L.ptr(t1), L.ptr(y1), L.ptr(a1),
                                    L.stream()))
    grads, bufs = [], [ybuf]
    for _ in range(2):
        gbuf, df = _canaried(cells, c, dt)
        L.check(fn["roialign_pool_bwd"](L.ptr(dy), L.ptr(a1), L.ptr(t1), L.ptr(sample), r, batch, hs, c, he, L.ptr(df),
                                        L.stream()))
        grads.append(df)
        bufs.append(gbuf)
    torch.cuda.synchronize()
    arg_canaries = bool((abuf[:8] == 200).all()) and bool((abuf[-8:] == 200).all())
    return dict(y0=y0, a0=a0, df0=df0, y1=y1, a1=a1, df1=grads[0], df1_again=grads[1], intact=_intact(bufs) and arg_canaries)


def _seeded_dy(seed, r, extract, c):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((r * (extract[0] // 2) * (extract[1] // 2) * (extract[2] // 2), c), generator=g)


def _check(res, nan=False):
    assert res["intact"]
    assert torch.equal(res["a1"], res["a0"])
    if nan:
        assert torch.allclose(res["y1"].float(), res["y0"].float(), rtol=0, atol=0, equal_nan=True)
        assert torch.allclose(res["df1"].float(), res["df0"].float(), rtol=0, atol=0, equal_nan=True)
    else:
        assert torch.equal(_bits(res["y1"]), _bits(res["y0"]))                   # bit for bit
        assert torch.equal(res["df1"], res["df0"])                               # as numbers
    assert torch.equal(_bits(res["df1"]), _bits(res["df1_again"]))               # reruns: identical bits


# ---- 1. the fused kernels against the two-call chain ---------------------------------------------------------------------------
@pytest.mark.parametrize("c,bf16", [(1, False), (12, False), (32, False), (40, False), (8, True), (40, True)])
@pytest.mark.parametrize("name", GEOMETRIES)
def test_fused_equals_the_chain(name, c, bf16):
    """aniso's extract (4, 6, 2) pools to (2, 3, 1); empty has no box (no launch forward, one memset backward); C = 1 takes the
    scalar lanes, 12 and 40 the 16-byte lanes with a partial wave."""
    z = _case(name)
    geo = _geometry(z)
    vol = torch.from_numpy(R.seeded_volume(70 + c, z["_batch"], z["_size"], c)).reshape(-1, c)
    res = _both(geo, vol, _seeded_dy(71 + c, geo["boxes"].shape[0], z["_extract"], c), bf16)
    _check(res)
    if geo["boxes"].shape[0] == 0:
        assert res["y1"].shape[0] == 0 and bool((res["df1"] == 0).all())
    else:
        assert float(res["df1"].float().abs().sum()) > 0
        assert int(res["a1"].max()) <= 7 and int(res["a1"].max()) > 0


def test_constant_volume_every_tie_goes_to_child_0():
    """Boxes whose sample positions are multiples of 1/2 (step (stop - start) / 7 = 1/2): every weight is dyadic, every sample
    of a constant volume is the constant exactly, all 8 children tie."""
    boxes = torch.tensor([[[0., 1., 1.5], [3.5, 4.5, 5.0]], [[1.5, 0., 0.5], [5.0, 3.5, 4.0]]])
    geo = dict(size=(6, 6, 6), extract=(8, 8, 8), batch=1, boxes=boxes, sample=torch.zeros(2, dtype=torch.int32))
    for bf16, c in ((False, 12), (True, 8)):
        vol = torch.full((216, c), -1.75)
        res = _both(geo, vol, _seeded_dy(5, 2, (8, 8, 8), c), bf16)
        _check(res)
        assert bool((res["a1"] == 0).all()) and bool((res["y1"] == -1.75).all())


def test_a_nan_cell():
    z = _case("small8")
    geo = _geometry(z)
    for bf16, c in ((False, 12), (True, 8)):
        vol = torch.from_numpy(R.seeded_volume(90, z["_batch"], z["_size"], c)).reshape(-1, c).clone()
        touched = ~np.unpackbits(z["grad_zero_rows"])[:vol.shape[0]].astype(bool)     # (cells some sample reads)
        vol[int(np.flatnonzero(touched)[0]), 3] = float("nan")
        res = _both(geo, vol, _seeded_dy(91, geo["boxes"].shape[0], z["_extract"], c), bf16)
        _check(res, nan=True)
        assert bool(torch.isnan(res["y1"].float()).any()) and not bool(torch.isnan(res["y1"].float()[:, :3]).any())


def test_130_boxes_in_one_sample():
    """More boxes in a sample than one pass of the backward holds in LDS (128)."""
    g = torch.Generator().manual_seed(17)
    n = [130, 3]
    a = torch.rand((sum(n), 3), generator=g) * 2.0
    boxes = torch.stack([a, torch.clamp(a + 0.3 + torch.rand((sum(n), 3), generator=g) * 2.0, max=3.0)], 1)
    sample = torch.tensor([0] * n[0] + [1] * n[1], dtype=torch.int32)
    geo = dict(size=(4, 4, 4), extract=(4, 4, 4), batch=2, boxes=boxes, sample=sample)
    c = 4
    vol = torch.randn((2 * 64, c), generator=g)
    res = _both(geo, vol, _seeded_dy(18, sum(n), (4, 4, 4), c), False)
    _check(res)
    assert float(res["df1"][:64].abs().sum()) > 0 and float(res["df1"][64:].abs().sum()) > 0


def test_refusals_before_any_launch():
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.functional import _host3
    lib = L.lib()
    c, size, r = 8, (6, 5, 4), 2
    vol = torch.zeros((120, c), device=DEV)
    boxes = torch.tensor([[[0., 0., 0.], [3., 3., 3.]]] * r, device=DEV)
    sample = torch.zeros(r, dtype=torch.int32, device=DEV)
    table = torch.empty(r * (3 * 24 + 2 * 15), dtype=torch.int32, device=DEV)
    y = torch.full((r * 64, c), CANARY, device=DEV)
    arg = torch.full((r * 64, c), 200, dtype=torch.uint8, device=DEV)
    df = torch.full((120, c), CANARY, device=DEV)
    for extract in ((8, 7, 8), (3, 8, 8), (8, 8, 1)):
        he = _host3(extract)
        for sfx in ("", "_bf16"):
            rc = getattr(lib, "scn_roialign_pool_fwd" + sfx)(L.ptr(vol), 1, _host3(size), c, L.ptr(boxes), L.ptr(sample), r, he,
                                                              L.ptr(table), L.ptr(y), L.ptr(arg), L.stream())
            assert rc == L.EINVAL, (extract, sfx)
            rc = getattr(lib, "scn_roialign_pool_bwd" + sfx)(L.ptr(y), L.ptr(arg), L.ptr(table), L.ptr(sample), r, 1,
                                                              _host3(size), c, he, L.ptr(df), L.stream())
            assert rc == L.EINVAL, (extract, sfx)
    rc = lib.scn_roialign_pool_fwd_bf16(L.ptr(vol), 1, _host3(size), 12, L.ptr(boxes), L.ptr(sample), r, _host3((8, 8, 8)),
                                        L.ptr(table), L.ptr(y), L.ptr(arg), L.stream())
    assert rc == L.EINVAL and b"c % 8" in lib.scn_last_error_string()
    torch.cuda.synchronize()
    assert bool((y == CANARY).all()) and bool((arg == 200).all()) and bool((df == CANARY).all())      # nothing ran
    from sparse_rcnn_amd.functional import RoiAlignPoolFunction
    with pytest.raises(ValueError):
        RoiAlignPoolFunction.apply(vol, boxes, sample, 1, size, (8, 7, 8))


@pytest.mark.parametrize("bf16", [False, True])
def test_autograd_function_and_its_padding_boxes(bf16):
    from sparse_rcnn_amd.functional import DenseMaxPoolFunction, RoiAlignFunction, RoiAlignPoolFunction
    z = _case("small8")
    geo = _geometry(z)
    c, dt = 16, BF if bf16 else torch.float32
    boxes, sample, r = geo["boxes"].to(DEV), geo["sample"].to(DEV), geo["boxes"].shape[0]
    vol = torch.from_numpy(R.seeded_volume(95, z["_batch"], z["_size"], c)).reshape(-1, c).to(DEV, dt)
    a, b = vol.clone().requires_grad_(), vol.clone().requires_grad_()
    per = 64
    y = RoiAlignPoolFunction.apply(a, boxes, sample, z["_batch"], z["_size"], z["_extract"], r + 3)
    ref = DenseMaxPoolFunction.apply(RoiAlignFunction.apply(b, boxes, sample, z["_batch"], z["_size"], z["_extract"]), r,
                                     z["_extract"], r + 3)
    assert y.dtype == dt and tuple(y.shape) == ((r + 3) * per, c)
    assert torch.equal(_bits(y.detach()), _bits(ref.detach())) and bool((y[r * per:] == 0).all())
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(96)).to(DEV, dt)          # (the padding rows' part is dropped)
    y.backward(g)
    ref.backward(g)
    assert a.grad.dtype == dt and torch.equal(a.grad, b.grad)
    y1 = RoiAlignPoolFunction.apply(vol, boxes, sample, z["_batch"], z["_size"], z["_extract"])
    assert torch.equal(_bits(y1), _bits(y.detach()[:r * per]))


# ---- 2. the flatten ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("v,c", [(64, 8), (1, 5), (64, 3), (8, 1)])
def test_box_flatten_bit_equal_to_torch(v, c, relu):
    from sparse_rcnn_amd.functional import BoxFlattenFunction
    r = 3
    g = torch.Generator().manual_seed(v * 100 + c)
    x = torch.randn((r * v, c), generator=g)
    x[torch.rand(x.shape, generator=g) < 0.2] = 0.0                               # zeros, and the negatives randn brings
    dy = torch.randn((r, c * v), generator=g)
    a = x.to(DEV).requires_grad_()
    y = BoxFlattenFunction.apply(a, r, relu)
    y.backward(dy.to(DEV))
    ref = x.view(r, v, c).permute(0, 2, 1).reshape(r, c * v)                      # column ch V + s
    ref = torch.relu(ref) if relu else ref
    ref_grad = dy.view(r, c, v).permute(0, 2, 1).reshape(r * v, c)
    ref_grad = torch.where(x > 0, ref_grad, torch.zeros(())) if relu else ref_grad
    assert bool((x == 0).any()) and bool((x < 0).any())
    assert torch.equal(_bits(y.detach().cpu()), _bits(ref))
    assert torch.equal(_bits(a.grad.cpu()), _bits(ref_grad.contiguous()))


def test_box_flatten_nan_and_no_boxes():
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.functional import BoxFlattenFunction
    x = torch.tensor([[1.0, float("nan")], [-2.0, 3.0]], device=DEV)
    y = BoxFlattenFunction.apply(x, 1, True)
    assert torch.equal(torch.isnan(y), torch.tensor([[False, False, True, False]], device=DEV))
    assert y[0, 0] == 1 and y[0, 1] == 0 and y[0, 3] == 3
    empty = BoxFlattenFunction.apply(torch.zeros((0, 8), device=DEV, requires_grad=True), 0, True)
    assert empty.shape[0] == 0
    assert L.lib().scn_box_flatten_fwd(None, 0, 64, 8, 1, None, L.stream()) == L.OK
    assert L.lib().scn_box_flatten_bwd(None, None, 0, 64, 8, 1, None, L.stream()) == L.OK
    with pytest.raises(ValueError):
        BoxFlattenFunction.apply(torch.zeros((7, 8), device=DEV), 2, False)


# ---- 3. the branch -------------------------------------------------------------------------------------------------------------
def _branch_and_inputs(name, fused=True):
    from sparse_rcnn_amd.classhead import ReshapeClassBranch
    z = S.load_fixture(GOLDEN, name)
    branch = ReshapeClassBranch(z["_c"], float(z["stride"]), tuple(z["same_channels"]), (8,), 5, fused=fused).to(DEV)
    assert branch.load_reference_state_dict({k: torch.from_numpy(v) for k, v in z["params"].items()}) == ([], [])
    vol = torch.from_numpy(z["volume"]).to(DEV).reshape(-1, z["_c"]).requires_grad_()
    boxes = [torch.from_numpy(b).to(DEV) for b in z["bbox_batch"]]
    return z, branch, vol, boxes


@functools.lru_cache(maxsize=None)
def _branch_run(name, fused):
    z, branch, vol, boxes = _branch_and_inputs(name, fused)
    scores, selection = branch(vol, z["_size"], z["_batch"], boxes)
    scores.backward(torch.from_numpy(z["score_grad"]).to(DEV))
    grads = {k: p.grad.detach().clone() for k, p in branch.named_oracle_params().items()}
    return z, branch, scores.detach(), selection, vol.grad.detach(), grads


@pytest.mark.parametrize("name", ["small", "two_same"])
def test_reshape_class_branch_against_the_fixture(name):
    from sparse_rcnn_amd.classhead import slab_to_conv3d_weight
    z, branch, scores, (bbox, counts, size), vol_grad, grads = _branch_run(name, True)
    assert counts == [int(v) for v in z["counts"]] and tuple(size) == z["_size"]
    assert bbox.cpu().numpy().tobytes() == z["bbox_tensor"].tobytes()
    assert scores.dtype == torch.float32 and tuple(scores.shape) == tuple(z["scores"].shape)
    scale = float(np.abs(z["scores"]).max())
    err = float(np.abs(scores.cpu().numpy() - z["scores"]).max())
    print(f"[reshape class] {name}: scores max err {err:.2e} (scale {scale:.3g})")
    assert err <= SCORE_BAR * scale
    rel = R.rel_l2(vol_grad.cpu().numpy(), z["volume_grad"])
    print(f"[reshape class] {name}: volume gradient rel L2 {rel:.2e}")
    assert rel <= GRAD_BAR
    step = int(z["element_step"])
    for rk, own in branch.reference_key_map().items():
        g, ref = grads[own].cpu(), z["grad/" + rk]
        if g.dim() == 3:                                        # back to the reference's Conv3d layout
            g = slab_to_conv3d_weight(g, 3).contiguous()
        g = g.numpy().reshape(-1)
        rel = R.rel_l2(g if ref.size == g.size else g[::step], ref)
        print(f"[reshape class] {name}: {rk} gradient rel L2 {rel:.2e}")
        assert rel <= GRAD_BAR, rk


@pytest.mark.parametrize("name", ["small", "two_same"])
def test_fused_branch_equals_the_chain_branch(name):
    _, _, s1, _, vg1, g1 = _branch_run(name, True)
    _, b0, s0, _, vg0, g0 = _branch_run(name, False)
    assert not b0.fused
    assert torch.equal(_bits(s1), _bits(s0)) and torch.equal(vg1, vg0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k


def test_branch_without_boxes_and_its_buckets():
    z, branch, vol, boxes = _branch_and_inputs("small")
    counts = [int(v) for v in z["counts"]]
    with torch.no_grad():
        none, (bbox, got, _) = branch(vol, z["_size"], z["_batch"], [b[:0] for b in boxes])
        assert tuple(none.shape) == (0, 5) and none.dtype == torch.float32 and got == [0, 0] and tuple(bbox.shape) == (0, 2, 3)
        assert len(branch._md) == 0
        ref_scores, _ = branch(vol, z["_size"], z["_batch"], boxes)
        n_md = len(branch._md)
        assert n_md == 1
        # another R in the same bucket: no new Metadata; an R in another bucket: the same scores for the shared boxes
        fewer, _ = branch(vol, z["_size"], z["_batch"], [boxes[0][:2], boxes[1]])
        assert len(branch._md) == n_md
        extra = torch.from_numpy(np.tile(z["boxes"][:1], (32, 1, 1))).to(DEV)
        more, (_, more_counts, _) = branch(vol, z["_size"], z["_batch"], [boxes[0], torch.cat([boxes[1], extra])])
    assert len(branch._md) == n_md + 1 and more_counts == [counts[0], counts[1] + 32]
    assert branch.bucket(sum(counts)) == 32 and branch.bucket(sum(counts) + 32) == 64
    scale = float(np.abs(z["scores"]).max())
    assert float((more[:sum(counts)] - ref_scores).abs().max()) <= 1e-5 * scale
    keep = [0, 1] + list(range(counts[0], sum(counts)))
    assert float((fewer - ref_scores[keep]).abs().max()) <= 1e-5 * scale
    assert float((more[sum(counts):] - more[sum(counts):sum(counts) + 1]).abs().max()) == 0      # 32 copies of one box in sample 1


@pytest.mark.parametrize("storage", [torch.float32, BF])
def test_dense_class_branch_fused_pool_equals_the_pair(storage):
    from sparse_rcnn_amd.classhead import DenseClassBranch
    small = json.load(open(os.path.join(GOLDEN, "dense_class_small.json")))
    z = dict(np.load(os.path.join(GOLDEN, "dense_class_small.npz")))
    seed, batch, size = int(z["seed"]), int(z["batch"]), tuple(int(v) for v in z["size"])
    c = 16 if storage is BF else int(z["c"])                                     # (bf16 lanes: widths in multiples of 8)
    shapes = dict(small["keys"])
    shapes["input_conv_layer.0.0.0.weight"] = [8, c, 1, 1, 1]
    params = {k: torch.from_numpy(v) for k, v in R.seeded_params(shapes, seed).items()}
    counts, o, boxes = [int(v) for v in z["counts"]], 0, []
    for n in counts:
        boxes.append(torch.from_numpy(z["boxes"][o:o + n]).to(DEV))
        o += n
    got = {}
    for fused in (False, True):
        branch = DenseClassBranch(c, 8, 8, (8, 16), (8,), 5, storage=storage, fused_pool=fused).to(DEV)
        assert branch.load_reference_state_dict(params) == ([], [])
        vol = torch.from_numpy(R.seeded_volume(seed, batch, size, c)).to(DEV, storage).reshape(-1, c).requires_grad_()
        scores, (bbox, got_counts, _) = branch(vol, size, batch, boxes)
        assert got_counts == counts and bbox.cpu().numpy().tobytes() == z["bbox_tensor"].tobytes()
        scores.backward(torch.from_numpy(z["score_grad"]).to(DEV))
        got[fused] = (scores.detach(), vol.grad, {k: p.grad for k, p in branch.named_oracle_params().items()})
    assert not DenseClassBranch(12, 8).fused_pool                                # the default stays the pair
    assert torch.equal(_bits(got[True][0]), _bits(got[False][0])) and torch.equal(got[True][1], got[False][1])
    for k, g in got[False][2].items():
        assert torch.equal(got[True][2][k], g), k


def test_scenestep_with_the_reshaping_class_head():
    from sparse_rcnn_amd.classhead import ReshapeClassBranch
    from sparse_rcnn_amd.trainstep import SceneStep
    kw = dict(optimizer='adam', rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True)
    st = SceneStep('cfg3-rpn', dense_class=True, simple_class=True, **kw)
    cb = st.model.class_branch
    assert isinstance(cb, ReshapeClassBranch) and cb.fused and "RESHAPING class head" in st.describe()
    assert cb.output_conv_layer[0].nIn == st.model.rpn.width and cb.linear_layer[1].in_features == 512
    for _ in range(2):
        st.step()
        for loss in (*st.rpn_losses, st.mask_losses, st.class_losses, st.segmentation_losses):
            assert bool(torch.isfinite(loss))
    st.finish()
    assert st.class_out[0].shape[1] == 18 and st.class_out[0].shape[0] == torch.cat(st.class_out[3]).numel()
    m = st.model
    m.backbone(st.coords, st.feats, st.size, st.batch_size, metadata=None)
    interims = m.backbone.unet.interims
    m.run_rpn(interims)
    scores, _ = m.run_class(interims, [b.float().to(st.device) for b in st.gt_boxes])
    (g,) = torch.autograd.grad(scores.sum(), [dict(m.named_parameters())["rpn.stack.0.weight"]], allow_unused=True)
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
    # predict() and evaluate() return the key sets of the dense arm
    out = st.predict()
    st.finish()
    assert {"roi_bbox", "class", "class_propabilities", "mask", "segmentation_class"} <= set(out)
    n_kept = [int(b.shape[0]) for b in out["roi_bbox"]]
    assert sum(n_kept) > 0 and st.predict_out[0].shape == (sum(n_kept), 18)
    assert [tuple(c.shape) for c in out["class"]] == [(n,) for n in n_kept]
    combined, single = st.evaluate(score_threshold=0.5)
    dense = SceneStep('cfg3-rpn', dense_class=True, **kw)
    ref_out = dense.predict()
    ref_combined, ref_single = dense.evaluate(score_threshold=0.5)
    dense.finish()
    assert set(out) == set(ref_out) and set(combined) == set(ref_combined) and set(single) == set(ref_single)
    assert all(np.isfinite(v) or np.isnan(v) for v in combined.values())
