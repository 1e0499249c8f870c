"""Sample conversion on the MI355X (sparse_rcnn_amd/sample.py on scn_sample_stats / scn_sample_pack): every fixture the
reference's own convert_sample wrote comes out bit-equal in every output; at size (200 000 points, 40 instances, the reference's
training parameters) the device path equals the host restatement bit for bit, twice, with canaries behind every buffer the
kernels write; collate against the restated collate_fn; a SceneStep fed converted batches against one fed the restatement's
host outputs through the existing pack_gt_masks path."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sample_restate as R                                     # noqa: E402
from test_sample_cpu import FIXTURES, NAMES                    # noqa: E402

pytestmark = pytest.mark.gpu


def _device_convert(sample, kw, **extra):
    """convert_sample with the restatement's keywords (tests/sample_restate.py convert)."""
    from sparse_rcnn_amd.sample import Draws, convert_sample
    draws = Draws(kw["almost_orthonormal"], kw["sub_pixel_offset"], start_positions=kw.get("start_positions"),
                  color_noise=kw["color_noise"], normal_noise=kw["normal_noise"])
    return convert_sample(
        sample, spatial_size=kw["spatial_size"], instance_cutoff_threshold=kw["instance_cutoff_threshold"],
        color_noise_sigma=0.1 if kw["color_noise"] is not None else 0, common_color_noise=False,
        normal_noise_sigma=0.1 if kw["normal_noise"] is not None else 0, common_normal_noise=False, use_color=kw["use_color"],
        use_ones=kw["use_ones"], use_normal=kw["use_normal"], additional_bbox_pixel=kw["additional_bbox_pixel"],
        background_label=kw["background_label"], scale=kw["scale"], instance_label_keep=[1, 2],
        instance_label_mapper=kw["instance_label_mapper"], segmentation_label_mapper=kw["segmentation_label_mapper"],
        required_size_factor=kw["required_size_factor"], shift=kw["shift"], draws=draws, **extra)


def _assert_equal(out, want, where):
    """A convert_sample 9-tuple against a restatement / fixture dict, every output, bits and dtypes."""
    _, coords, feats, bbox, gt_mask, label, seg, augm, size = out
    mask = gt_mask.unpack(0) if not torch.is_tensor(gt_mask) else gt_mask
    got = dict(coords=coords, is_inside=augm["remaining_points"], features=feats, bbox=bbox, mask=mask, label=label, seg=seg,
               size=size, coords_shift=augm["coords_shift"], coords_projection=augm["coords_projection"])
    for k, v in want.items():
        g = got[k].cpu()
        assert g.dtype == v.dtype and g.shape == v.shape, (where, k, g.dtype, v.dtype, tuple(g.shape), tuple(v.shape))
        if v.dtype.is_floating_point:                          # bits, not values: -0.0 and NaN payloads count
            assert torch.equal(g.contiguous().view(torch.int32), v.contiguous().view(torch.int32)), (where, k)
        else:
            assert torch.equal(g, v), (where, k)


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_fixture_bit_equal(gpu, path):
    from sparse_rcnn_amd.loss import PackedMasks
    sample, kw, want, _ = R.load_fixture(path)
    out = _device_convert(("scene",) + sample, kw)
    assert out[0] == "scene" and isinstance(out[4], PackedMasks) and out[1].is_cuda and out[2].is_cuda
    _assert_equal(out, want, "packed")
    dense = _device_convert(sample, kw, dense_masks=True)          # the stored 5-tuple, the reference's bool [G, M]
    assert dense[0] is None and dense[4].dtype == torch.bool
    _assert_equal(dense, want, "dense")


def _training_mappers(n_raw=41):
    """Mappers shaped like the reference's (scannet_config: 41 raw ids -> 18 instance classes or -1, 20 segmentation classes
    or -100)."""
    rng = np.random.default_rng(0)
    inst = rng.integers(-1, 18, size=n_raw)
    inst[::5] = -1
    seg = rng.integers(0, 20, size=n_raw)
    seg[::7] = -100
    return torch.from_numpy(inst.astype(np.int64)), torch.from_numpy(seg.astype(np.int64))


def _training_kw(sample, seed, spatial_size, shift=None, random_cut=False, required_size_factor=None):
    """The reference's training parameters (scannet_config/run.py:941-984 var_params): threshold 0.8, no extra box pixels,
    scale 1 / 0.02, coord noise 0.1, per-point colour noise 0.1, no normal noise, random mirror / angle / offset."""
    from sparse_rcnn_amd.sample import draw_augmentation
    inst, seg = _training_mappers()
    torch.manual_seed(seed)
    d = draw_augmentation(coord_noise_sigma=0.1, theta=None, mirror=None, sub_pixel_offset=None)
    kw = dict(almost_orthonormal=d.almost_orthonormal, sub_pixel_offset=d.sub_pixel_offset, scale=1 / 0.02,
              spatial_size=spatial_size, shift=shift, start_positions=None, instance_cutoff_threshold=0.8, color_noise=None,
              normal_noise=None, use_color=True, use_ones=True, use_normal=True, additional_bbox_pixel=0, background_label=-100,
              instance_label_mapper=inst, segmentation_label_mapper=seg, required_size_factor=required_size_factor)
    if random_cut:                                             # the draw the reference makes next, restated on the host
        aug = R.matmul3(sample[0], d.almost_orthonormal * kw["scale"])
        discrete = (aug + (-aug.min(0).values + d.sub_pixel_offset)).long()
        size = torch.tensor(spatial_size)
        kw["start_positions"], _, _ = R.random_cut_out(discrete, size, [0, 0, 0])
    m = int(R.convert(*sample, **kw)["coords"].shape[0])
    kw["color_noise"] = 0.1 * torch.randn((m, 3))
    return kw


CANARY = 0x5A5A5A5A


def _with_tail(numel, dtype, dev, tail=256):
    raw = torch.full((numel * torch.empty((), dtype=dtype).element_size() // 4 + tail,), CANARY, dtype=torch.int32, device=dev)
    return raw, raw[:raw.numel() - tail].view(dtype)


def _tail_intact(raw, tail=256):
    return bool((raw[-tail:] == CANARY).all())


def test_at_size_fixed_cut_equals_restatement_twice_with_canaries(gpu):
    from sparse_rcnn_amd import _lib as L
    from sparse_rcnn_amd.synthetic import make_raw_sample
    from sparse_rcnn_amd.voxelize import _augment_coords, _f32xn, _i32x3
    sample = make_raw_sample(200_000, 40, seed=1)
    n, n_inst = sample[0].shape[0], 40
    kw = _training_kw(sample, seed=5, spatial_size=(320, 320, 160), shift=0)
    want = R.convert(*sample, **kw)
    m, g = want["coords"].shape[0], want["mask"].shape[0]
    print(f"[at size] N {n} M {m} instances kept {g} of {n_inst}, points in kept masks {int(want['mask'].sum())}")
    blas = sample[0] @ (kw["almost_orthonormal"] * kw["scale"])
    print(f"[at size] elements of this CPU's BLAS product that differ from the stated association: "
          f"{int((blas != R.matmul3(sample[0], kw['almost_orthonormal'] * kw['scale'])).sum())} of {blas.numel()}")
    assert n > 190_000 and m > 50_000 and g >= 5
    dev_sample = tuple(t.to(gpu) for t in sample[:4]) + (sample[4],)
    a = _device_convert(dev_sample, kw)
    b = _device_convert(dev_sample, kw)
    _assert_equal(a, want, "run 1")
    _assert_equal(b, want, "run 2")
    assert torch.equal(a[4].words, b[4].words)
    w = (m + 31) // 32
    words = a[4].words[:g * w].view(g, w)
    if m % 32:                                                 # zero bits beyond M
        assert int(((words[:, -1].to(torch.int64) & 0xFFFFFFFF) >> (m % 32)).sum()) == 0
    # the entry points themselves on buffers with canary tails behind every output
    lib = L.lib()
    coords, colors, normals, ids = dev_sample[:4]
    _, _, _, _, ex = _augment_coords(coords, rot_and_scale=kw["almost_orthonormal"] * kw["scale"],
                                     sub_pixel_offset=kw["sub_pixel_offset"], spatial_size=kw["spatial_size"], shift=0)
    stats_raw, stats = _with_tail((n_inst + 1) * 8, torch.int32, gpu)
    bad_raw, bad = _with_tail(1, torch.int32, gpu)
    L.check(lib.scn_sample_stats(L.ptr(ex["discrete"]), L.ptr(ex["table"]), L.ptr(ids), n, n_inst, _i32x3(ex["start"]),
                                 L.ptr(stats), L.ptr(bad), L.stream()))
    feats_raw, feats = _with_tail(m * 7, torch.float32, gpu)
    seg_raw, seg = _with_tail(m, torch.int64, gpu)
    words_raw, wbuf = _with_tail(g * w, torch.int32, gpu)
    from sparse_rcnn_amd.sample import select_instances
    kept, _, _ = select_instances(stats.cpu().view(n_inst + 1, 8), sample[4], 0.8, kw["instance_label_mapper"], 0)
    slot = torch.full((n_inst + 1,), -1, dtype=torch.int32)
    slot[kept] = torch.arange(len(kept), dtype=torch.int32)
    seg_table = torch.cat([kw["segmentation_label_mapper"][sample[4]], torch.tensor([-100])]).to(gpu)
    noise = kw["color_noise"].to(gpu)
    L.check(lib.scn_sample_pack(L.ptr(ex["rows"]), m, L.ptr(colors), L.ptr(normals), L.ptr(ids), n_inst,
                                _f32xn(kw["almost_orthonormal"], 9), L.ptr(noise), 1, None, 0, 1, 1, 1, L.ptr(feats),
                                L.ptr(seg_table), L.ptr(seg), L.ptr(slot.to(gpu)), g, L.ptr(wbuf), L.stream()))
    torch.cuda.synchronize()
    for name, raw in (("stats", stats_raw), ("n_bad", bad_raw), ("features", feats_raw), ("seg", seg_raw), ("words", words_raw)):
        assert _tail_intact(raw), name
    assert int(bad[0]) == 0 and len(kept) == g
    assert torch.equal(feats.view(m, 7).cpu().view(torch.int32), want["features"].view(torch.int32))
    assert torch.equal(seg.cpu(), want["seg"]) and torch.equal(wbuf, a[4].words[:g * w])
    # instance ids outside 0 .. I are counted on the device and refused by convert_sample
    broken = ids.clone()
    broken[::1000] = n_inst + 3
    broken[5] = -1
    L.check(lib.scn_sample_stats(L.ptr(ex["discrete"]), L.ptr(ex["table"]), L.ptr(broken), n, n_inst, _i32x3(ex["start"]),
                                 L.ptr(stats), L.ptr(bad), L.stream()))
    assert int(bad[0]) == int(((broken < 0) | (broken > n_inst)).sum())
    with pytest.raises(L.ScnError, match="instance id"):
        _device_convert(dev_sample[:3] + (broken, sample[4]), kw)
    with pytest.raises(L.ScnError, match="instances"):
        _device_convert(dev_sample[:4] + (torch.zeros(L.SAMPLE_MAX_INSTANCES + 1, dtype=torch.int64),), kw)


def test_random_cut_with_given_and_drawn_start_equals_restatement(gpu):
    """The reference's training path (shift None, spatial_size = the training crop): start positions given, and drawn by
    convert_sample itself from the generator (random_cut_start on the device voxels) under the seed the restatement used."""
    from sparse_rcnn_amd.sample import Draws, convert_sample
    from sparse_rcnn_amd.synthetic import make_raw_sample
    sample = make_raw_sample(200_000, 40, seed=2)
    kw = _training_kw(sample, seed=18, spatial_size=(128, 128, 64), random_cut=True)
    want = R.convert(*sample, **kw)
    print(f"[random cut] start {kw['start_positions'].tolist()} M {want['coords'].shape[0]} kept {want['mask'].shape[0]}")
    assert want["coords"].shape[0] > 5000 and want["mask"].shape[0] >= 2
    _assert_equal(_device_convert(sample, kw), want, "given start")
    # drawn here: the same seed, the same order of draws -> the same start, noise and outputs
    inst, seg = _training_mappers()
    torch.manual_seed(18)
    out = convert_sample(sample, spatial_size=(128, 128, 64), instance_cutoff_threshold=0.8, color_noise_sigma=0.1,
                         common_color_noise=False, normal_noise_sigma=0, common_normal_noise=False, use_color=True, use_ones=True,
                         use_normal=True, additional_bbox_pixel=0, background_label=-100, scale=1 / 0.02,
                         instance_label_mapper=inst, segmentation_label_mapper=seg, max_empty_border_size_divisor=None,
                         shift=None, sub_pixel_offset=None, coord_noise_sigma=0.1, theta=None, mirror=None)
    _assert_equal(out, want, "drawn start")
    assert torch.equal(out[7]["color_shift"], kw["color_noise"])


@pytest.mark.parametrize("n_samples", [2, 12])
def test_collate_equals_restated_collate_fn(gpu, n_samples):
    from sparse_rcnn_amd.sample import collate
    from sparse_rcnn_amd.synthetic import make_raw_sample
    raw = [make_raw_sample(15_000, 12, seed=20 + i) for i in range(3)]
    outs, wants = [], []
    for i in range(n_samples):
        sample = raw[i % 3]
        kw = _training_kw(sample, seed=40 + i, spatial_size=(64, 64, 32), random_cut=True, required_size_factor=16)
        kw["instance_cutoff_threshold"] = 0.5
        wants.append(R.convert(*sample, **kw))
        outs.append(_device_convert((f"s{i}",) + sample, kw))
    want = R.collate(wants)
    batch = collate(outs)
    coords_batch, feats, size, batch_size, splits = batch["data"]
    assert coords_batch.is_cuda and feats.is_cuda and batch["gt_segmentation"].is_cuda
    assert torch.equal(coords_batch.cpu(), want["coords_batch"]) and torch.equal(feats.cpu(), want["features"])
    assert torch.equal(size, want["spatial_size"]) and batch_size == n_samples and splits == want["batch_splits"]
    assert torch.equal(batch["gt_segmentation"].cpu(), want["gt_segmentation"]) and batch["id"] == tuple(f"s{i}" for i in range(n_samples))
    assert sum(wt["mask"].shape[0] for wt in wants) > 0
    for s, wt in enumerate(wants):
        assert torch.equal(batch["gt_bbox"][s].cpu(), wt["bbox"]) and torch.equal(batch["gt_label"][s].cpu(), wt["label"])
        assert torch.equal(batch["gt_mask"].unpack(s).cpu(), wt["mask"])


def _step_batches(gpu):
    """One converted scene (no cut-out, moved by 2 voxels: without a shift the reference's spatial size is the LARGEST coordinate,
    which leaves the points on that face outside [0, size); size rounded to 32: the 4-level network's factor 8 times the class branch's 4) and its twin from the
    restatement."""
    from sparse_rcnn_amd.sample import collate
    from sparse_rcnn_amd.synthetic import make_raw_sample
    sample = make_raw_sample(120_000, 30, seed=3)
    kw = _training_kw(sample, seed=13, spatial_size=None, shift=2, required_size_factor=32)
    want = R.convert(*sample, **kw)
    batch = collate([_device_convert(sample, kw)])
    w = R.collate([want])
    twin = dict(id=("twin",), data=(w["coords_batch"].to(gpu), w["features"].to(gpu), w["spatial_size"], 1, w["batch_splits"]),
                gt_bbox=[b.to(gpu) for b in w["gt_bbox"]], gt_label=[l.to(gpu) for l in w["gt_label"]],
                gt_mask=[mk.to(gpu) for mk in w["gt_mask"]], gt_segmentation=w["gt_segmentation"].to(gpu),
                batch_splits=w["batch_splits"], augmentation=({},))
    return batch, twin, want, kw, sample


def test_scene_step_on_converted_batches(gpu):
    from sparse_rcnn_amd.sample import collate
    from sparse_rcnn_amd.trainstep import SceneStep
    batch, twin, want, kw, sample = _step_batches(gpu)
    print(f"[step] M {want['coords'].shape[0]} G {want['mask'].shape[0]} size {want['size'].tolist()}")
    assert want["mask"].shape[0] >= 5
    flags = dict(optimizer="adam", rpn_loss=True, mask_loss=True, class_loss=True, segmentation_loss=True, prefetch=False, lr=1e-4)
    losses, grads = [], []
    for b in (batch, twin):
        st = SceneStep("cfg3-rpn", batches=[b], **flags)
        st.step()
        st.finish()
        losses.append([st.rpn_losses[0], st.rpn_losses[1], st.mask_losses, st.class_losses, st.segmentation_losses])
        grads.append(torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in st.flat.params]))
        if b is batch:
            assert "converted sample" in st.describe()
            st.step()
            for v in (st.rpn_losses[0], st.rpn_losses[1], st.mask_losses, st.class_losses, st.segmentation_losses):
                assert bool(torch.isfinite(v.detach()).all())
            pred = st.predict()
            st.finish()
            assert len(pred["roi_bbox"]) == 1 and pred["segmentation_class"].shape[0] == want["coords"].shape[0]
            combined, _ = st.evaluate(score_threshold=0.0)
            st.finish()
            assert combined and any(key.startswith("mask_AP") for key in combined), sorted(combined)
        del st
    for name, x, y in zip(("rpn_score", "rpn_bbox", "mask", "class", "segmentation"), *losses):
        x, y = x.detach().cpu(), y.detach().cpu()
        print(f"[step] {name}: {float(x):.7f} | twin {float(y):.7f}")
        assert bool(torch.isfinite(x)) and torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert bool(grads[0].abs().sum() > 0) and torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))
    # a spatial size the network's levels do not divide is refused, with the way out
    odd = collate([_device_convert(sample, dict(kw, required_size_factor=8))])
    assert any(int(v) % 32 for v in odd["data"][2])
    with pytest.raises(ValueError, match="required_size_factor=32"):
        SceneStep("cfg3-rpn", batches=[odd], **flags)
    odd = collate([_device_convert(sample, dict(kw, required_size_factor=None))])
    assert any(int(v) % 8 for v in odd["data"][2])
    with pytest.raises(ValueError, match="required_size_factor=8"):
        SceneStep("cfg3-rpn", batches=[odd], optimizer="adam", rpn_loss=True, mask_loss=True, prefetch=False)
    with pytest.raises(ValueError, match="batches"):
        SceneStep("cfg3", batches=[batch])
