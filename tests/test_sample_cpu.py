"""Sample conversion, host side (no GPU): the restatement tests/sample_restate.py is pinned bit for bit to the fixtures the
reference's own convert_sample wrote (tests/golden/make_sample_golden.py); the host helpers of sparse_rcnn_amd/sample.py --
draws, random cut-out start, instance selection, collate -- are checked against fixtures and restatement; the C entry points
refuse bad sizes with a status code before anything is launched."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sample_restate as R                                     # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "sample_*.npz")))
NAMES = [os.path.basename(f)[7:-4] for f in FIXTURES]


def test_fixture_set_covers_the_deciding_cases():
    assert set(NAMES) >= {"fixcut", "fixcut_shift", "fixcut_small", "fixcut_empty", "nocut", "nocut_nokeep"}
    seen = dict(threshold=False, zero_points=False, all_outside=False, mapper_drop=False, no_instance_points=False,
                none_kept=False, odd_pixel=False, zero_pixel=False, common_noise=False, point_noise=False, no_normal=False,
                size_factor=False, mirror=False, empty=False)
    for f in FIXTURES:
        (coords, colors, normals, ids, raw), kw, want, st = R.load_fixture(f)
        n_inst = raw.shape[0]
        inside = want["is_inside"]
        cnt = torch.bincount(ids, minlength=n_inst + 1)
        cin = torch.bincount(ids[inside], minlength=n_inst + 1)
        thr = kw["instance_cutoff_threshold"]
        seen["threshold"] |= bool(((cnt[:n_inst] > 0) & (cin[:n_inst].float() / cnt[:n_inst].float() == thr)).any()) and thr == 0.5
        seen["zero_points"] |= bool((cnt[:n_inst] == 0).any())
        seen["all_outside"] |= bool(((cnt[:n_inst] > 0) & (cin[:n_inst] == 0)).any())
        if kw["instance_label_mapper"] is not None:
            dropped = kw["instance_label_mapper"][raw] < 0
            seen["mapper_drop"] |= bool((dropped & (cin[:n_inst] == cnt[:n_inst]) & (cnt[:n_inst] > 0)
                                         & (kw["segmentation_label_mapper"][raw] >= 0)).any())
        seen["no_instance_points"] |= bool(cin[n_inst] > 0)
        seen["none_kept"] |= want["bbox"].shape == (0, 2, 3) and want["mask"].shape[0] == 0 and want["mask"].shape[1] > 0
        seen["odd_pixel"] |= kw["additional_bbox_pixel"] % 2 == 1
        seen["zero_pixel"] |= kw["additional_bbox_pixel"] == 0
        for k in ("color_noise", "normal_noise"):
            if kw[k] is not None:
                seen["common_noise"] |= kw[k].dim() == 1
                seen["point_noise"] |= kw[k].dim() == 2
        seen["no_normal"] |= not kw["use_normal"]
        seen["size_factor"] |= kw["required_size_factor"] is not None
        seen["mirror"] |= st["mirror"] is True and float(torch.linalg.det(kw["almost_orthonormal"].double())) < 0
        seen["empty"] |= want["coords"].shape[0] == 0
    assert all(seen.values()), seen


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_restatement_equals_reference_fixture(path):
    sample, kw, want, _ = R.load_fixture(path)
    got = R.convert(*sample, **kw)
    assert set(want) == set(got)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, k
        assert torch.equal(got[k], v), k


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_draw_augmentation_reproduces_the_stored_draws(path):
    from sparse_rcnn_amd.sample import draw_augmentation
    _, kw, want, st = R.load_fixture(path)
    torch.manual_seed(st["seed"])
    d = draw_augmentation(coord_noise_sigma=st["coord_noise_sigma"], theta=st["theta"], mirror=st["mirror"],
                          sub_pixel_offset=st["fixed_sub_pixel_offset"], color_noise_sigma=st["color_noise_sigma"],
                          common_color_noise=st["common_color_noise"], normal_noise_sigma=st["normal_noise_sigma"],
                          common_normal_noise=st["common_normal_noise"], use_color=kw["use_color"], use_normal=kw["use_normal"],
                          num_kept=want["coords"].shape[0])
    assert torch.equal(d.almost_orthonormal, kw["almost_orthonormal"])
    assert torch.equal(d.sub_pixel_offset, kw["sub_pixel_offset"])
    for got, ref in ((d.color_noise, kw["color_noise"]), (d.normal_noise, kw["normal_noise"])):
        assert (got is None) == (ref is None)
        if ref is not None:
            assert torch.equal(got, ref)


def _stats_table(out_coords, is_inside, ids, n_inst):
    """What scn_sample_stats computes, in numpy."""
    big, small = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    st = np.zeros((n_inst + 1, 8), np.int32)
    st[:, 2:5], st[:, 5:8] = big, small
    ids, is_inside, oc = ids.numpy(), is_inside.numpy(), out_coords.numpy()
    ids_in = ids[is_inside]
    for i in range(n_inst + 1):
        st[i, 0] = (ids == i).sum()
        sel = oc[ids_in == i]
        st[i, 1] = len(sel)
        if len(sel):
            st[i, 2:5], st[i, 5:8] = sel.min(0), sel.max(0)
    return torch.from_numpy(st)


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_host_selection_from_exact_counts_equals_fixture(path):
    from sparse_rcnn_amd.sample import select_instances
    (coords, colors, normals, ids, raw), kw, want, _ = R.load_fixture(path)
    stats = _stats_table(want["coords"], want["is_inside"], ids, raw.shape[0])
    kept, label, bbox = select_instances(stats, raw, kw["instance_cutoff_threshold"], kw["instance_label_mapper"],
                                         kw["additional_bbox_pixel"])
    assert torch.equal(label, want["label"]) and label.dtype == torch.int64
    assert bbox.dtype == torch.float32 and bbox.shape == want["bbox"].shape and torch.equal(bbox, want["bbox"])
    ids_in = ids[want["is_inside"]]
    mask = torch.stack([ids_in == i for i in kept]) if len(kept) else torch.zeros((0, len(ids_in)), dtype=torch.bool)
    assert torch.equal(mask, want["mask"])


@pytest.mark.parametrize("seed", range(12))
def test_random_cut_start_equals_restated_random_cut_out(seed):
    from sparse_rcnn_amd.sample import random_cut_start
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 4000))
    extent = rng.integers(4, 200, size=3)
    pts = torch.from_numpy(rng.integers(0, extent, size=(n, 3)).astype(np.int64))
    size = [int(v) for v in rng.integers(8, 160, size=3)]
    divisor = [None, 4, 8, 3][seed % 4]
    border = [0, 0, 0] if divisor is None else [s // divisor for s in size]
    torch.manual_seed(100 + seed)
    start_ref, inside_ref, coords_ref = R.random_cut_out(pts, torch.tensor(size), border)
    after_ref = torch.rand(1)
    torch.manual_seed(100 + seed)
    start = random_cut_start(pts.to(torch.int32), size, border)
    after = torch.rand(1)
    assert start.dtype == torch.int64 and torch.equal(start, start_ref)
    assert torch.equal(after, after_ref)                       # the same number of draws was taken from the generator
    moved = pts - start
    inside = ((moved >= 0) & (moved < torch.tensor(size))).all(1)
    assert torch.equal(inside, inside_ref) and torch.equal(moved[inside], coords_ref)


def _pack_words(mask):
    """bool [G, M] -> PackedMasks words (int32 bit patterns), in numpy."""
    g, m = mask.shape
    w = (m + 31) // 32
    bits = np.zeros((g, w * 32), np.uint8)
    bits[:, :m] = mask.numpy()
    words = np.packbits(bits.reshape(g, w, 32), axis=-1, bitorder="little").view("<u4").reshape(g * w)
    return torch.from_numpy(words.view(np.int32).copy()) if g * w else torch.zeros(1, dtype=torch.int32)


def test_collate_on_host_samples_equals_restated_collate_fn():
    from sparse_rcnn_amd.loss import PackedMasks
    from sparse_rcnn_amd.sample import collate
    outs, samples, dense = [], [], []
    for i, path in enumerate(FIXTURES):
        sample, kw, _, _ = R.load_fixture(path)
        if not (kw["use_normal"] and kw["use_ones"]):
            continue                                           # (one feature width per batch)
        o = R.convert(*sample, **kw)
        outs.append(o)
        packed = PackedMasks(_pack_words(o["mask"]), [o["mask"].shape[0]], [o["mask"].shape[1]])
        assert torch.equal(packed.unpack(0), o["mask"])
        base = (f"scene{i}", o["coords"], o["features"], o["bbox"])
        tail = (o["label"], o["seg"], dict(coords_shift=o["coords_shift"]), o["size"])
        samples.append(base + (packed,) + tail)
        dense.append(base + (o["mask"],) + tail)
    assert len(outs) >= 3
    want = R.collate(outs)
    for kind, batch in (("packed", collate(samples)), ("dense", collate(dense))):
        coords_batch, feats, size, batch_size, splits = batch["data"]
        assert coords_batch.dtype == torch.int64 and torch.equal(coords_batch, want["coords_batch"])
        assert torch.equal(feats, want["features"]) and torch.equal(size, want["spatial_size"])
        assert batch_size == want["batch_size"] and splits == want["batch_splits"] == batch["batch_splits"]
        assert torch.equal(batch["gt_segmentation"], want["gt_segmentation"])
        assert batch["id"] == tuple(s[0] for s in samples) and len(batch["augmentation"]) == len(outs)
        for s, o in enumerate(outs):
            assert torch.equal(batch["gt_bbox"][s], o["bbox"]) and torch.equal(batch["gt_label"][s], o["label"])
            got = batch["gt_mask"].unpack(s) if kind == "packed" else batch["gt_mask"][s]
            assert torch.equal(got, o["mask"])
        if kind == "packed":
            assert batch["gt_mask"].n_gt == [o["mask"].shape[0] for o in outs]
            assert batch["gt_mask"].n_points == want["batch_splits"]


def test_make_raw_sample_is_a_stored_sample():
    from sparse_rcnn_amd.synthetic import make_raw_sample
    a = make_raw_sample(6000, 9, seed=4)
    b = make_raw_sample(6000, 9, seed=4)
    coords, colors, normals, ids, raw = a
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    n = coords.shape[0]
    assert abs(n - 6000) < 600 and coords.dtype == colors.dtype == normals.dtype == torch.float32
    assert colors.shape == normals.shape == (n, 3) and ids.shape == (n,) and ids.dtype == raw.dtype == torch.int64
    assert raw.shape == (9,) and int(ids.min()) >= 0 and int(ids.max()) == 9 and int((ids < 9).sum()) > 0
    assert float(colors.abs().max()) <= 1 and torch.allclose(normals.norm(dim=1), torch.ones(n), atol=1e-5)


def test_entry_points_refuse_bad_sizes_before_any_launch():
    from sparse_rcnn_amd import _lib as L
    lib = L.load()
    buf = (C.c_int32 * 64)()
    start = (C.c_int32 * 3)(0, 0, 0)
    p = C.addressof(buf)
    assert lib.scn_sample_stats(p, p, p, 0, 3, start, p, p, None) == L.EINVAL                     # N = 0
    assert lib.scn_sample_stats(p, p, p, 8, L.SAMPLE_MAX_INSTANCES + 1, start, p, p, None) == L.ESIZE
    assert b"instances" in lib.scn_last_error_string()
    assert lib.scn_sample_stats(p, p, None, 8, 3, start, p, p, None) == L.EINVAL
    rot = (C.c_float * 9)()
    args = (p, p, p, 3, rot, None, 0, None, 0, 1, 1, 1, p, p, p, p, 1, p, None)
    assert lib.scn_sample_pack(p, -1, *args) == L.EINVAL
    assert lib.scn_sample_pack(p, 0, *args) == L.OK                                                # M = 0: nothing to do
    assert lib.scn_sample_pack(p, 8, p, p, p, L.SAMPLE_MAX_INSTANCES + 1, *args[4:]) == L.ESIZE
    assert lib.scn_sample_pack(p, 8, p, p, p, 3, rot, None, 0, None, 0, 1, 1, 1, None, p, p, p, 1, p, None) == L.EINVAL
