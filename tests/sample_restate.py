"""Host restatement (torch CPU) of the reference's sample conversion with every random draw given: ndsis/data/
sparse_augmentation.py convert_sample (:250-313) = augment_coords + augment_features + get_masks + get_bbox +
get_semantic_segmentation_labels, ndsis/data/data.py collate_fn (:88-115), and random_cut_out (:50-78) with its aliasing
assignment applied to a clone.  tests/test_sample_cpu.py pins it to the fixtures tests/golden/sample_*.npz (written by the
reference's own code) bit for bit; the GPU tests compare the device path against it at sizes no fixture covers."""
from fractions import Fraction

import numpy as np
import torch


def _fma32(a, b, c):
    """Correctly rounded fp32 a * b + c, elementwise (numpy fp32 arrays).  The product of two fp32 values is exact in fp64; the
    fp64 sum is rounded once more on the way to fp32, which can only go wrong when it lands exactly half-way between two fp32
    values: those elements (normally none) are redone in rational arithmetic."""
    a, b, c = np.broadcast_arrays(a, b, c)
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    out = s.astype(np.float32)
    tie = np.isfinite(s) & ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000)
    for i in zip(*np.nonzero(tie)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = sorted((float(np.nextafter(out[i], np.float32(-np.inf))), float(np.nextafter(out[i], np.float32(np.inf)))))
        out[i] = min((lo, float(out[i]), hi), key=lambda v: (abs(Fraction(v) - exact), int(np.float32(v).view(np.int32)) & 1))
    return out


def matmul3(points, matrix):
    """[N, 3] @ [3, 3] in fp32 with the association torch's CPU matmul was found to use for K = 3 where the fixtures were
    written, and which the device kernels state (scn_vox_project): fma(z, R2j, fma(y, R1j, x * R0j)).  Spelled out because a
    BLAS picks its kernel by the machine it runs on: the last bit of `points @ matrix` is not the same on every CPU."""
    p, r = points.cpu().numpy().astype(np.float32), matrix.cpu().numpy().astype(np.float32)
    t = p[:, 0:1] * r[0:1, :]
    t = _fma32(p[:, 1:2], r[1:2, :], t)
    t = _fma32(p[:, 2:3], r[2:3, :], t)
    return torch.from_numpy(t).to(points.device)


def random_cut_out(discrete_coords, size, max_border):
    """random_cut_out as written, but `is_inside[is_inside] = remaining_inside` through a clone of the index (the original
    line raises on current torch).  Draws from torch's CPU generator.  -> (start_positions, is_inside, inside_coords)"""
    num_dims = len(size)
    order = torch.multinomial(torch.ones(num_dims), num_dims)
    start = torch.zeros(num_dims, dtype=torch.int64)
    is_inside = torch.ones(discrete_coords.shape[0], dtype=torch.bool)
    inside = discrete_coords.clone()
    for dim in order:
        if not len(inside):
            break
        lo = inside[:, dim].min() - max_border[dim]
        hi = inside[:, dim].max() + 1 - size[dim] + max_border[dim]
        if hi <= lo:
            start[dim] = lo
            inside[:, dim] -= start[dim]
        else:
            start[dim] = torch.randint(int(lo), int(hi), ())
            inside[:, dim] -= start[dim]
            remaining = (0 <= inside[:, dim]) & (inside[:, dim] < size[dim])
            inside = inside[remaining]
            is_inside[is_inside.clone()] = remaining
    return start, is_inside, inside


def convert(coords, colors, normals, instance_ids, labels_raw, *, almost_orthonormal, sub_pixel_offset, scale,
            spatial_size=None, shift=None, start_positions=None, instance_cutoff_threshold, color_noise=None, normal_noise=None,
            use_color=True, use_ones=True, use_normal=True, additional_bbox_pixel=0, background_label=-100,
            instance_label_mapper=None, segmentation_label_mapper=None, required_size_factor=None):
    """-> dict(coords, is_inside, features, bbox, mask (bool [G, M]), label, seg, size, coords_shift, coords_projection).
    color_noise / normal_noise: the reference's feature_shift ([3] or [M, 3]) or None.  Runs where `coords` lives: on device
    tensors this is what the reference's `load_using_gpu` mode does (the same torch operators, a Python loop and a host wait per
    instance), which tools/sample_bench.py times."""
    dev = coords.device
    on = lambda t: (t if t is None else torch.as_tensor(t).to(dev))               # noqa: E731
    ortho = torch.as_tensor(almost_orthonormal, dtype=torch.float32).to(dev)
    sub_pixel_offset, color_noise, normal_noise = on(sub_pixel_offset), on(color_noise), on(normal_noise)
    labels_raw, instance_label_mapper, segmentation_label_mapper = on(labels_raw), on(instance_label_mapper), on(segmentation_label_mapper)
    projection = ortho * scale
    aug = matmul3(coords, projection) if coords.device.type == "cpu" else coords @ projection
    complete_shift = -aug.min(0).values + torch.as_tensor(sub_pixel_offset, dtype=torch.float32)
    discrete = (aug + complete_shift).long()
    if spatial_size is not None:
        size = torch.as_tensor(spatial_size, dtype=torch.int64).expand(3).to(dev)
        if shift is not None:
            start = torch.as_tensor(-shift, dtype=torch.int64).expand(3).to(dev)
            is_inside = ((discrete >= 0) & (discrete < size)).all(-1)
        else:
            start = torch.as_tensor(start_positions, dtype=torch.int64).to(dev)
            moved = discrete - start
            is_inside = ((moved >= 0) & (moved < size)).all(-1)
        out_coords = (discrete - start)[is_inside]
        complete_shift = complete_shift - start.float()
    else:
        size = discrete.max(0).values
        is_inside = torch.ones(discrete.shape[0], dtype=torch.bool, device=dev)
        out_coords = discrete
        if shift is not None:
            out_coords = discrete + shift
            size = size + 2 * shift
            complete_shift = complete_shift + shift
    m = out_coords.shape[0]
    parts = []
    if use_color:
        c = colors[is_inside]
        parts.append(c if color_noise is None else c + color_noise)
    if use_ones:
        parts.append(torch.ones((m, 1), device=dev))
    if use_normal:
        nr = matmul3(normals[is_inside], ortho) if dev.type == "cpu" else normals[is_inside] @ ortho
        parts.append(nr if normal_noise is None else nr + normal_noise)
    features = torch.cat(parts, 1) if parts else torch.zeros((m, 0), device=dev)

    ids_in = instance_ids[is_inside]
    kept, labels = [], []
    for i in range(labels_raw.shape[0]):
        label = int(labels_raw[i]) if instance_label_mapper is None else int(instance_label_mapper[labels_raw[i]])
        if instance_label_mapper is not None and label < 0:
            continue
        member = instance_ids == i
        ratio = is_inside[member].float().mean()
        if ratio > instance_cutoff_threshold:
            kept.append(i)
            labels.append(label)
    mask = torch.stack([ids_in == i for i in kept]) if kept else torch.zeros((0, m), dtype=torch.bool, device=dev)
    if kept:
        bbox = torch.stack([torch.stack((out_coords[r].min(0).values, out_coords[r].max(0).values + 1)) for r in mask]).float()
    else:
        bbox = torch.zeros((0, 2, 3), device=dev)
    if additional_bbox_pixel:
        bbox = bbox + torch.tensor([[-additional_bbox_pixel / 2], [additional_bbox_pixel / 2]], device=dev)
    seg_raw = labels_raw if segmentation_label_mapper is None else segmentation_label_mapper[labels_raw]
    seg = torch.cat([seg_raw, torch.tensor([background_label], device=dev)])[ids_in]
    if required_size_factor is not None:
        size = required_size_factor * (-(-size // required_size_factor))
    return dict(coords=out_coords, is_inside=is_inside, features=features, bbox=bbox, mask=mask,
                label=torch.tensor(labels, dtype=torch.int64, device=dev), seg=seg, size=size.cpu(), coords_shift=complete_shift.cpu(),
                coords_projection=projection.cpu())


def collate(outs):
    """collate_fn's layout over a list of `convert` outputs -> dict(coords_batch [sum M, 4], features, spatial_size, batch_size,
    batch_splits, gt_bbox, gt_label, gt_mask (lists), gt_segmentation)."""
    coords_batch = torch.cat([torch.nn.functional.pad(o["coords"], (0, 1), value=i) for i, o in enumerate(outs)])
    return dict(coords_batch=coords_batch, features=torch.cat([o["features"] for o in outs]),
                spatial_size=torch.stack([o["size"] for o in outs]).max(0).values, batch_size=len(outs),
                batch_splits=[len(o["coords"]) for o in outs], gt_bbox=[o["bbox"] for o in outs],
                gt_label=[o["label"] for o in outs], gt_mask=[o["mask"] for o in outs],
                gt_segmentation=torch.cat([o["seg"] for o in outs]))


def load_fixture(path):
    """A tests/golden/sample_*.npz -> (sample tensors, convert() keywords, expected outputs, conversion settings)."""
    import numpy as np
    z = np.load(path)
    t = lambda k: torch.from_numpy(z[k])                                        # noqa: E731
    opt = lambda k: (t(k) if z[k].size else None)                               # noqa: E731
    num = lambda k: (None if int(z["has_" + k]) == 0 else z[k].item())          # noqa: E731
    sample = (t("coords"), t("colors"), t("normals"), t("instance_ids"), t("labels_raw"))
    size = None if int(z["has_spatial_size"]) == 0 else tuple(int(v) for v in z["spatial_size"])
    kw = dict(almost_orthonormal=t("almost_orthonormal"), sub_pixel_offset=t("sub_pixel_offset"), scale=float(z["scale"]),
              spatial_size=size, shift=num("shift"), instance_cutoff_threshold=float(z["instance_cutoff_threshold"]),
              color_noise=opt("color_noise"), normal_noise=opt("normal_noise"), use_color=bool(z["use_color"]),
              use_ones=bool(z["use_ones"]), use_normal=bool(z["use_normal"]),
              additional_bbox_pixel=z["additional_bbox_pixel"].item(), background_label=int(z["background_label"]),
              instance_label_mapper=opt("instance_label_mapper"), segmentation_label_mapper=opt("segmentation_label_mapper"),
              required_size_factor=num("required_size_factor"))
    want = {k[4:]: t(k) for k in z.files if k.startswith("out_")}
    settings = dict(seed=int(z["seed"]), coord_noise_sigma=float(z["coord_noise_sigma"]), theta=num("theta"), mirror=num("mirror"),
                    fixed_sub_pixel_offset=num("fixed_sub_pixel_offset"), color_noise_sigma=float(z["color_noise_sigma"]),
                    common_color_noise=bool(z["common_color_noise"]), normal_noise_sigma=float(z["normal_noise_sigma"]),
                    common_normal_noise=bool(z["common_normal_noise"]))
    return sample, kw, want, settings
