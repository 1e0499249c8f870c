"""Generates tests/golden/sample_*.npz by RUNNING the reference's own convert_sample (ndsis/data/sparse_augmentation.py) on
the CPU, on seeded samples.  Run in the build container only:

    python tests/golden/make_sample_golden.py

The random objects the reference draws (distortion matrix, sub-pixel offset, colour / normal noise) are stored as inputs next
to the outputs, with the seed that produced them: the RNG is replayed for the matrix and the offset, the noise is the
`color_shift` / `normals_shift` the reference itself reports.  The instance ids are laid out AFTER a first run has shown which
points the cut-out keeps, so that the cases that decide the selection rules are hit exactly (see `layout`).
random_cut_out raises on this torch (see make_vox_golden.py): that path has no fixture.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
from ndsis.data import sparse_augmentation as SA                               # noqa: E402
import sample_restate as R                                                      # noqa: E402

INSTANCE_MAPPER = torch.tensor([-1, 0, 1, 2, -1, 3, 4, 5, 6, 7])               # raw label -> instance class or -1 (dropped)
SEGMENTATION_MAPPER = torch.tensor([0, 2, 3, 4, 1, 5, 6, 7, 8, 9])              # raw label -> segmentation class (keeps 0 and 4)


def layout(rng, inside, n_inst, x):
    """Instance ids 0 .. n_inst (n_inst = none) and raw labels for the cases that decide the rules:
      0  exactly half of its points inside (ratio 0.5: dropped at threshold 0.5, strictly greater)
      1  no point at all (0 / 0 = NaN: dropped)
      2  every point outside the cut (dropped; all inside when nothing is cut)
      3  all inside, raw label 4: the instance mapper sends it to -1, the segmentation mapper keeps it
      4..  balls of 0.7 m around random points (some inside, some cut through, some outside); the rest has id n_inst."""
    n = len(inside)
    ids = np.full(n, n_inst, np.int64)
    free_in = list(np.flatnonzero(inside))
    free_out = list(np.flatnonzero(~inside))
    rng.shuffle(free_in)
    rng.shuffle(free_out)
    take = lambda pool, k: [pool.pop() for _ in range(min(k, len(pool)))]      # noqa: E731
    half = take(free_out, 40)
    if half:
        ids[half + take(free_in, len(half))] = 0
    ids[take(free_out, 60)] = 2
    ids[take(free_in, 50)] = 3
    rest = np.array(free_in + free_out)
    centres = [free_in[k] if (k % 3 and k < len(free_in)) else rest[rng.integers(len(rest))] for k in range(n_inst - 4)]
    for k in reversed(range(n_inst - 4)):                                       # (the lower id wins where two balls meet)
        near = rest[np.linalg.norm(x[rest] - x[centres[k]], axis=1) < 0.7]
        ids[near] = 4 + k
    labels_raw = rng.integers(1, 10, size=n_inst)
    labels_raw[labels_raw == 4] = 5
    labels_raw[3] = 4
    return ids, labels_raw.astype(np.int64)


def case(name, seed, n, n_inst, *, scale, spatial_size, shift, threshold, mappers=True, **conv):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(0, 6, size=(n // 2, 3)) * np.array([1, 1, 0.02]),
                          rng.uniform(0, 6, size=(n - n // 2, 3)) * np.array([1, 0.02, 0.5])]).astype(np.float32)
    colors = (rng.integers(0, 256, size=(n, 3)) / 127.5 - 1).astype(np.float32)
    normals = rng.normal(size=(n, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    coords = torch.from_numpy(pts)
    aug_kw = dict(coord_noise_sigma=conv.pop("coord_noise_sigma", 0.05), theta=conv.pop("theta", None),
                  mirror=conv.pop("mirror", None), sub_pixel_offset=conv.pop("sub_pixel_offset", None))
    params = dict(spatial_size=spatial_size, instance_cutoff_threshold=threshold, color_noise_sigma=0.1,
                  common_color_noise=False, normal_noise_sigma=0, common_normal_noise=False, use_color=True, use_ones=True,
                  use_normal=True, additional_bbox_pixel=0, background_label=-100, instance_label_keep=None,
                  instance_label_mapper=INSTANCE_MAPPER if mappers else None,
                  segmentation_label_mapper=SEGMENTATION_MAPPER if mappers else None, required_size_factor=None,
                  scale=scale, max_empty_border_size_divisor=None, shift=shift)
    params.update(conv)
    # first run: which points does the cut-out keep under this seed?
    torch.manual_seed(seed)
    _, inside, _, _, _ = SA.augment_coords(coords, scale=scale, spatial_size=spatial_size, max_empty_border_size_divisor=None,
                                           shift=shift, **aug_kw)
    ids, labels_raw = layout(rng, inside.numpy(), n_inst, pts)
    sample = ("scene", coords, torch.from_numpy(colors), torch.from_numpy(normals), torch.from_numpy(ids),
              torch.from_numpy(labels_raw))
    torch.manual_seed(seed)
    (_, out_coords, features, bbox, mask, label, seg, augm, size) = SA.convert_sample(sample, **params, **aug_kw)
    # replay: the matrix and the offset
    torch.manual_seed(seed)
    ortho = SA.get_coord_distortion_matrix(torch.float32, coord_noise_sigma=aug_kw["coord_noise_sigma"], theta=aug_kw["theta"],
                                           mirror=aug_kw["mirror"])
    offset = torch.rand(3) if aug_kw["sub_pixel_offset"] is None else torch.as_tensor(aug_kw["sub_pixel_offset"],
                                                                                       dtype=torch.float32).expand(3)
    assert torch.equal(ortho * scale, augm["coords_projection"])
    noise = lambda k: (augm[k].numpy() if k in augm and augm[k].dim() else np.zeros(0, np.float32))   # noqa: E731
    opt = lambda v: (np.array(0) if v is None else np.array(v))                # noqa: E731
    has = lambda v: np.array(int(v is not None))                                # noqa: E731
    none = np.zeros(0, np.int64)
    store = dict(
        coords=pts, colors=colors, normals=normals, instance_ids=ids, labels_raw=labels_raw,
        almost_orthonormal=ortho.numpy(), sub_pixel_offset=offset.numpy(), color_noise=noise("color_shift"),
        normal_noise=noise("normals_shift"), seed=np.array(seed), scale=np.array(scale),
        has_spatial_size=has(spatial_size), spatial_size=opt(spatial_size), has_shift=has(shift), shift=opt(shift),
        instance_cutoff_threshold=np.array(threshold), use_color=np.array(params["use_color"]),
        use_ones=np.array(params["use_ones"]), use_normal=np.array(params["use_normal"]),
        additional_bbox_pixel=np.array(params["additional_bbox_pixel"]), background_label=np.array(-100),
        instance_label_mapper=INSTANCE_MAPPER.numpy() if mappers else none,
        segmentation_label_mapper=SEGMENTATION_MAPPER.numpy() if mappers else none,
        has_required_size_factor=has(params["required_size_factor"]), required_size_factor=opt(params["required_size_factor"]),
        coord_noise_sigma=np.array(aug_kw["coord_noise_sigma"]), has_theta=has(aug_kw["theta"]), theta=opt(aug_kw["theta"]),
        has_mirror=has(aug_kw["mirror"]), mirror=opt(aug_kw["mirror"]),
        has_fixed_sub_pixel_offset=has(aug_kw["sub_pixel_offset"]), fixed_sub_pixel_offset=opt(aug_kw["sub_pixel_offset"]),
        color_noise_sigma=np.array(params["color_noise_sigma"]), common_color_noise=np.array(params["common_color_noise"]),
        normal_noise_sigma=np.array(params["normal_noise_sigma"]), common_normal_noise=np.array(params["common_normal_noise"]),
        out_coords=out_coords.numpy(), out_is_inside=augm["remaining_points"].numpy(), out_features=features.numpy(),
        out_bbox=bbox.numpy(), out_mask=mask.numpy(), out_label=label.numpy(), out_seg=seg.numpy(),
        out_size=torch.as_tensor(size).numpy(), out_coords_shift=augm["coords_shift"].numpy(),
        out_coords_projection=augm["coords_projection"].numpy())
    path = os.path.join(HERE, f"sample_{name}.npz")
    np.savez_compressed(path, **store)
    # the restatement agrees with what was just written (the CPU test checks this again from the file)
    smp, kw, want, _ = R.load_fixture(path)
    got = R.convert(*smp, **kw)
    for k, v in want.items():
        assert torch.equal(got[k], v) and got[k].dtype == v.dtype, (name, k)
    counts = np.bincount(ids, minlength=n_inst + 1)
    print(name, "M", tuple(out_coords.shape), "G", len(label), "kept labels", label.tolist(), "size", torch.as_tensor(size).tolist(),
          "ratio0", float(inside.numpy()[ids == 0].mean()) if counts[0] else None, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    # fixed cut-out; instance 0 exactly at the threshold; mirror on (the normals' matrix is not a pure rotation); common
    # colour noise, per-point normal noise
    case("fixcut", 11, 3000, 10, scale=25.0, spatial_size=(96, 96, 48), shift=0, threshold=0.5, mirror=True,
         common_color_noise=True, normal_noise_sigma=0.05)
    # fixed cut-out moved by 4, odd additional_bbox_pixel, per-point colour noise, no normals, fixed theta
    case("fixcut_shift", 12, 3000, 9, scale=20.0, spatial_size=(64, 96, 48), shift=4, threshold=0.5, additional_bbox_pixel=3,
         use_normal=False, theta=0.7)
    # no cut-out: required_size_factor rounds the size; no mappers; common normal noise, no colour noise; fixed offset
    case("nocut", 13, 2500, 8, scale=30.0, spatial_size=None, shift=None, threshold=0.8, mappers=False, required_size_factor=16,
         additional_bbox_pixel=2, color_noise_sigma=0, normal_noise_sigma=0.1, common_normal_noise=True, sub_pixel_offset=0)
    # no cut-out with a shift; a threshold nothing passes: [0, 2, 3] boxes and [0, M] masks; no ones column
    case("nocut_nokeep", 14, 2000, 7, scale=30.0, spatial_size=None, shift=3, threshold=1.0, use_ones=False,
         required_size_factor=8, mirror=False)
    # a cut-out that keeps no point at all: M = 0
    case("fixcut_empty", 15, 3000, 12, scale=25.0, spatial_size=(32, 48, 32), shift=0, threshold=0.3, additional_bbox_pixel=0,
         common_color_noise=True, normal_noise_sigma=0.02, common_normal_noise=True, mirror=True)
    # a small cut-out: most instances are entirely outside
    case("fixcut_small", 16, 3000, 12, scale=25.0, spatial_size=(64, 64, 48), shift=0, threshold=0.3, additional_bbox_pixel=1,
         common_color_noise=True, normal_noise_sigma=0.02, common_normal_noise=True)
