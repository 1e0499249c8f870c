"""Training batches from stored scene samples, on the device.

`convert_sample` is ndsis/data/sparse_augmentation.py ``convert_sample`` (:250-313) and `collate` is ndsis/data/data.py
``collate_fn`` (:88-115).  The coordinate part is `voxelize.augment_coords` (scn_vox_*); this module adds what makes the batch
a supervised one -- the feature tensor, the instances that survive the cut-out with their boxes, point masks and labels, the
per-point segmentation labels, the rounded spatial size -- on scn_sample_stats / scn_sample_pack (csrc/scn_sample.hip).

Every random number of the reference is an input (`Draws`).  `draw_augmentation` / `random_cut_start` draw them on the host
with torch's CPU generator, by the reference's calls in the reference's order, so one ``torch.manual_seed`` gives the
reference's values; `convert_sample(..., draws=None)` calls them itself at the points where the reference draws.

Host waits of one `convert_sample`: the kept-row count (augment_coords' own) and ONE copy of the (I + 1) x 8 instance table,
queued before that count is waited for.  The random cut-out adds the three small reads of `random_cut_start`.
DEVIATION: ``augmentation['remaining_points']`` stays on the device (the reference copies N bools to the host per sample).
"""
from __future__ import annotations

import math

import torch

from . import _lib as L
from .loss import PackedMasks
from .voxelize import _augment_coords, _f32xn, _i32x3

__all__ = ["Draws", "draw_augmentation", "random_cut_start", "convert_sample", "collate", "join_packed_masks"]


class Draws:
    """The random objects of one conversion, host tensors: `almost_orthonormal` fp32 [3,3] (get_coord_distortion_matrix),
    `sub_pixel_offset` fp32 [3], `start_positions` int64 [3] or None (random cut-out), `color_noise` / `normal_noise` = the
    reference's `feature_shift` (sigma * randn; [3] common or [M,3] in kept-row order) or None.  A None that the conversion
    needs is drawn when the reference would draw it."""

    def __init__(self, almost_orthonormal, sub_pixel_offset, start_positions=None, color_noise=None, normal_noise=None):
        self.almost_orthonormal = torch.as_tensor(almost_orthonormal, dtype=torch.float32).reshape(3, 3)
        self.sub_pixel_offset = torch.as_tensor(sub_pixel_offset, dtype=torch.float32).expand(3).clone()
        self.start_positions = None if start_positions is None else torch.as_tensor(start_positions, dtype=torch.int64)
        self.color_noise = None if color_noise is None else torch.as_tensor(color_noise, dtype=torch.float32)
        self.normal_noise = None if normal_noise is None else torch.as_tensor(normal_noise, dtype=torch.float32)


def _distortion_matrix(dtype, coord_noise_sigma, theta, mirror):
    """get_coord_distortion_matrix (sparse_augmentation.py:9-38): randn(3,3), then randint(0,2) if mirror is None, then rand()
    if theta is None (multinomial if theta is a list)."""
    m = torch.eye(3, dtype=dtype) + torch.randn((3, 3), dtype=dtype) * coord_noise_sigma
    m[0, 0] *= (torch.randint(0, 2, ()) * 2 - 1) if mirror is None else (-1 if mirror else 1)
    if theta is None:
        angle = torch.rand((), dtype=dtype) * 2 * math.pi
    else:
        angle = torch.tensor(theta, dtype=dtype)
        if angle.numel() > 1:
            angle = angle[torch.ones_like(angle).multinomial(1)[0]]
    c, s = torch.cos(angle), torch.sin(angle)
    return m @ torch.tensor([[c, s, 0.], [-s, c, 0.], [0., 0., 1.]])


def _feature_noise(sigma, common, m, dtype=torch.float32):
    """augment_single_feature's draw (:136-142); None when the reference draws nothing."""
    if not sigma:
        return None
    return sigma * torch.randn((3,) if common else (m, 3), dtype=dtype)


def draw_augmentation(*, coord_noise_sigma, theta=None, mirror=None, sub_pixel_offset=None, color_noise_sigma=0,
                      common_color_noise=False, normal_noise_sigma=0, common_normal_noise=False, use_color=True,
                      use_normal=True, num_kept=None, dtype=torch.float32):
    """Host helper: the draws of one `convert_sample` from torch's CPU generator, in the reference's order -- distortion matrix,
    `torch.rand(3)` (unless sub_pixel_offset is given), then the colour and the normal noise.  Fixed theta / mirror /
    sub_pixel_offset pass through.  Per-point noise has one row per KEPT point: it is drawn here when `num_kept` is given and
    otherwise left to `convert_sample`, which draws it after the cut-out (also the place of the random cut-out's own draws,
    which precede the noise in the reference: pass no num_kept on that path)."""
    ortho = _distortion_matrix(dtype, coord_noise_sigma, theta, mirror)
    offset = torch.rand((3,), dtype=dtype) if sub_pixel_offset is None else sub_pixel_offset
    d = Draws(ortho, offset)
    if use_color and color_noise_sigma and (common_color_noise or num_kept is not None):
        d.color_noise = _feature_noise(color_noise_sigma, common_color_noise, num_kept, dtype)
    if use_normal and normal_noise_sigma and (common_normal_noise or num_kept is not None):
        if use_color and color_noise_sigma and d.color_noise is None:
            raise ValueError("the per-point colour noise is drawn before the normal noise: give num_kept, or leave both to "
                             "convert_sample")
        d.normal_noise = _feature_noise(normal_noise_sigma, common_normal_noise, num_kept, dtype)
    return d


def random_cut_start(discrete_coords, size, max_border):
    """The start positions `random_cut_out` (sparse_augmentation.py:50-78) draws: a random order of the dimensions by
    `torch.multinomial(ones, num_dims)`, then per dimension the min / max of the voxels that survived the dimensions before,
    `min_start = min - max_border`, `max_start = max + 1 - size + max_border`, and `torch.randint(min_start, max_start, ())`
    where that range is not empty (else min_start, and nothing is cut along that dimension).  max_border[d] =
    size[d] // max_empty_border_size_divisor (0 without a divisor).  -> int64 [num_dims] on the host.

    discrete_coords: integer [N, num_dims], host or device.  On the device the min / max / count of a dimension come back in
    ONE small copy per dimension -- three host reads per sample; the draw depends on them, so they cannot be deferred.  The
    draws use torch's CPU generator whatever the device.

    The reference's own function raises on current torch (`is_inside[is_inside] = remaining_inside` writes through an index of
    itself), so no fixture can pin this path: the tests check it against a restatement of `random_cut_out` with that line
    applied to a clone, under the same seed."""
    num_dims = len(size)
    size = [int(s) for s in size]
    border = [int(b) for b in max_border]
    order = torch.multinomial(torch.ones(num_dims), num_dims)
    start = torch.zeros(num_dims, dtype=torch.int64)
    d = discrete_coords
    alive = None
    big = torch.iinfo(d.dtype).max
    for dim in order.tolist():
        col = d[:, dim]
        if alive is None:
            lo, hi, cnt = col.min(), col.max(), torch.tensor(col.shape[0], dtype=col.dtype, device=col.device)
        else:
            lo = torch.where(alive, col, torch.full_like(col, big)).min()
            hi = torch.where(alive, col, torch.full_like(col, -big)).max()
            cnt = alive.sum().to(col.dtype)
        lo, hi, cnt = (int(v) for v in torch.stack([lo, hi, cnt]).cpu().tolist())         # the host read of this dimension
        if cnt == 0:
            break
        min_start = lo - border[dim]
        max_start = hi + 1 - size[dim] + border[dim]
        if max_start <= min_start:
            start[dim] = min_start
        else:
            start[dim] = torch.randint(min_start, max_start, ())
            moved = col - int(start[dim])
            inside = (moved >= 0) & (moved < size[dim])
            alive = inside if alive is None else (alive & inside)
    return start


def _ceil_div(a, b):
    return -(-a // b)


def select_instances(stats, labels_raw, instance_cutoff_threshold, instance_label_mapper, additional_bbox_pixel):
    """get_masks' selection (:208-234) and get_bbox (:188-205) from the exact per-instance table, on the host.
    stats int32 [I + 1, 8] CPU (scn_sample_stats), labels_raw int64 [I] CPU.
    -> (kept instance ids int64 [G] ascending, their labels int64 [G], boxes fp32 [G, 2, 3])."""
    n_inst = labels_raw.shape[0]
    st = stats[:n_inst].to(torch.int64)
    if instance_label_mapper is not None:
        labels = torch.as_tensor(instance_label_mapper).cpu()[labels_raw]
        candidate = labels >= 0
    else:
        labels = labels_raw
        candidate = torch.ones(n_inst, dtype=torch.bool)
    ratio = st[:, 1].float() / st[:, 0].float()            # .float().mean() of a bool column: one fp32 division; 0 / 0 = NaN
    keep = candidate & (ratio > instance_cutoff_threshold)
    kept = torch.nonzero(keep).reshape(-1)
    if bool((st[kept, 1] == 0).any()):
        raise ValueError("an instance without a point inside the cut-out was kept (instance_cutoff_threshold < 0): it has no box")
    if kept.numel():
        boxes = torch.stack((st[kept, 2:5], st[kept, 5:8] + 1), 1).float()
    else:
        boxes = torch.zeros((0, 2, 3), dtype=torch.int64).float()
    if additional_bbox_pixel:
        boxes += boxes.new_tensor([[-additional_bbox_pixel / 2], [additional_bbox_pixel / 2]])
    return kept, labels[keep], boxes


def convert_sample(sample, *, spatial_size, instance_cutoff_threshold, color_noise_sigma, common_color_noise,
                   normal_noise_sigma, common_normal_noise, use_color, use_ones, use_normal, additional_bbox_pixel,
                   background_label, scale, instance_label_keep=None, instance_label_mapper=None,
                   segmentation_label_mapper=None, device=None, required_size_factor=None,
                   max_empty_border_size_divisor=None, shift=None, sub_pixel_offset=None, coord_noise_sigma=0, theta=None,
                   mirror=None, draws=None, dense_masks=False, batch_index=0):
    """The reference's `convert_sample` with its keyword names.  sample = (scene_id, coords, colors, normals, instance_ids,
    semantic_instance_labels_raw) or the stored 5-tuple without the id: coords / colors / normals fp32 [N,3], instance_ids int64
    [N] with values 0 .. I (I = no instance), labels_raw int64 [I].  The per-point tensors go to the device (`device`, default
    the current one) if they are not there; labels_raw is a few hundred values and is used on the host (a device tensor costs
    a copy and a wait).

    draws: a `Draws` (every None in it that is needed is drawn in place), or None: `draw_augmentation` from coord_noise_sigma /
    theta / mirror / sub_pixel_offset here.  With a `Draws`, those four keywords are not read.
    Cut-out: spatial_size and shift -> fixed; spatial_size alone -> random (`draws.start_positions`, else `random_cut_start`
    with max_empty_border_size_divisor); spatial_size None -> none.  (Without a cut-out the reference's spatial size is the
    LARGEST voxel coordinate + 2 shift: with shift None or 0 the points on the far faces lie outside [0, size), and a network fed
    with them refuses the batch -- use shift >= 1, or a cut-out, as the reference's configurations do.)

    -> the reference's 9-tuple (scene_id, coords int64 [M,3], features fp32 [M,C], gt_bbox fp32 [G,2,3], gt_mask, gt_label int64
    [G], segmentation labels int64 [M], augmentation dict, spatial_size int64 CPU [3]), tensors on the device.  gt_mask is a
    `loss.PackedMasks` of one sample (the dense [G, M] matrix never exists); dense_masks=True unpacks it to the reference's
    bool [G, M].  instance_label_keep is accepted and ignored, as in the reference.  A point whose instance id is outside
    0 .. I raises (the reference's index error)."""
    if len(sample) == 6:
        scene_id, coords, colors, normals, instance_ids, labels_raw = sample
    else:
        scene_id = None
        coords, colors, normals, instance_ids, labels_raw = sample
    lib = L.lib()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    coords = coords.to(dev, torch.float32).contiguous()
    colors = colors.to(dev, torch.float32).contiguous() if use_color else None
    normals = normals.to(dev, torch.float32).contiguous() if use_normal else None
    instance_ids = instance_ids.to(dev, torch.int64).contiguous()
    labels_raw = torch.as_tensor(labels_raw).to("cpu", torch.int64)
    n, n_inst = coords.shape[0], labels_raw.shape[0]
    if instance_ids.shape[0] != n:
        raise ValueError("instance_ids: one id per point required")
    if n_inst > L.SAMPLE_MAX_INSTANCES:
        raise L.ScnError(f"{n_inst} instances: scn_sample_stats holds at most {L.SAMPLE_MAX_INSTANCES}")
    if draws is None:
        draws = draw_augmentation(coord_noise_sigma=coord_noise_sigma, theta=theta, mirror=mirror,
                                  sub_pixel_offset=sub_pixel_offset, use_color=False, use_normal=False)
    rot_and_scale = draws.almost_orthonormal * scale

    start_positions = None
    if spatial_size is not None and shift is None:
        if draws.start_positions is not None:
            start_positions = draws.start_positions
        else:
            size3 = [int(s) for s in torch.as_tensor(spatial_size).expand(3).tolist()]
            border = [0, 0, 0] if max_empty_border_size_divisor is None else [s // max_empty_border_size_divisor for s in size3]

            def start_positions(discrete):
                draws.start_positions = random_cut_start(discrete, size3, border)
                return draws.start_positions

    table_buf = torch.empty((n_inst + 1) * 8 + 8, dtype=torch.int32, device=dev)

    def queue_stats(discrete, table, start):
        L.check(lib.scn_sample_stats(L.ptr(discrete), L.ptr(table), L.ptr(instance_ids), n, n_inst, _i32x3(start),
                                     L.ptr(table_buf), table_buf.data_ptr() + (n_inst + 1) * 32, L.stream()))

    rows4, is_inside, size_out, complete_shift, extra = _augment_coords(
        coords, rot_and_scale=rot_and_scale, sub_pixel_offset=draws.sub_pixel_offset, spatial_size=spatial_size, shift=shift,
        start_positions=start_positions, batch_index=batch_index, before_wait=queue_stats)
    rows = extra["rows"]
    m = int(rows.shape[0])
    host = table_buf.cpu()                                   # the one host wait of this module
    if int(host[(n_inst + 1) * 8]):
        raise L.ScnError(f"{int(host[(n_inst + 1) * 8])} points carry an instance id outside 0 .. {n_inst}")
    stats = host[:(n_inst + 1) * 8].view(n_inst + 1, 8)
    kept, gt_label, boxes = select_instances(stats, labels_raw, instance_cutoff_threshold, instance_label_mapper,
                                             additional_bbox_pixel)
    g = int(kept.numel())
    slot_of = torch.full((n_inst + 1,), -1, dtype=torch.int32)
    slot_of[kept] = torch.arange(g, dtype=torch.int32)
    seg_raw = labels_raw if segmentation_label_mapper is None else torch.as_tensor(segmentation_label_mapper).cpu()[labels_raw]
    seg_table = torch.nn.functional.pad(seg_raw.to(torch.int64), (0, 1), value=background_label)

    # the noise of the kept rows: drawn now if it was not given (the reference draws it here, colour first)
    if use_color and color_noise_sigma and draws.color_noise is None:
        draws.color_noise = _feature_noise(color_noise_sigma, common_color_noise, m)
    if use_normal and normal_noise_sigma and draws.normal_noise is None:
        draws.normal_noise = _feature_noise(normal_noise_sigma, common_normal_noise, m)
    cn = draws.color_noise if (use_color and color_noise_sigma) else None
    nn_ = draws.normal_noise if (use_normal and normal_noise_sigma) else None
    for name, t in (("color_noise", cn), ("normal_noise", nn_)):
        if t is not None and tuple(t.shape) not in ((3,), (m, 3)):
            raise ValueError(f"{name}: [3] or [{m}, 3] (one row per kept point) required, got {tuple(t.shape)}")
    cn_dev = None if cn is None else cn.to(dev).contiguous()
    nn_dev = None if nn_ is None else nn_.to(dev).contiguous()

    c = (3 if use_color else 0) + (1 if use_ones else 0) + (3 if use_normal else 0)
    features = torch.empty((m, c), dtype=torch.float32, device=dev)
    seg = torch.empty((m,), dtype=torch.int64, device=dev)
    w = (m + 31) // 32
    words = torch.empty(max(g * w, 1), dtype=torch.int32, device=dev)
    slot_dev, seg_table_dev = slot_of.to(dev), seg_table.to(dev)
    L.check(lib.scn_sample_pack(
        L.ptr(rows), m, L.ptr(colors), L.ptr(normals), L.ptr(instance_ids), n_inst,
        _f32xn(draws.almost_orthonormal, 9), L.ptr(cn_dev), int(cn is not None and cn.dim() == 2), L.ptr(nn_dev),
        int(nn_ is not None and nn_.dim() == 2), int(bool(use_color)), int(bool(use_ones)), int(bool(use_normal)),
        L.ptr(features) if c else 0, L.ptr(seg_table_dev), L.ptr(seg), L.ptr(slot_dev), g, L.ptr(words), L.stream()))
    gt_mask = PackedMasks(words, [g], [m])
    if dense_masks:
        gt_mask = gt_mask.unpack(0)

    augmentation = dict(coords_projection=rot_and_scale, coords_shift=complete_shift)
    if use_color:
        augmentation["color_shift"] = cn if cn is not None else torch.zeros(())
    if use_normal:
        augmentation["normals_shift"] = nn_ if nn_ is not None else torch.zeros(())
    augmentation["remaining_points"] = is_inside
    if required_size_factor is not None:
        size_out = required_size_factor * _ceil_div(size_out, required_size_factor)
    return (scene_id, rows4[:, :3], features, boxes.to(dev), gt_mask, gt_label.to(dev), seg, augmentation, size_out)


def join_packed_masks(masks):
    """Several PackedMasks (one or more samples each) as one, samples in order: the words lie back to back."""
    masks = list(masks)
    n_gt = [g for mk in masks for g in mk.n_gt]
    n_points = [p for mk in masks for p in mk.n_points]
    parts = [mk.words[:mk.word_offsets[-1]] for mk in masks]
    out = PackedMasks(None, n_gt, n_points)
    if out.word_offsets[-1]:
        out.words = torch.cat(parts)
    else:
        ref = masks[0].words if masks else torch.zeros(1, dtype=torch.int32)
        out.words = torch.zeros(1, dtype=torch.int32, device=ref.device)
    return out


def collate(samples):
    """`collate_fn` (data.py:88-115) over `convert_sample` outputs -> dict with the reference's keys: `id`, `data` =
    (coords_batch int64 [sum M, 4] with the sample index in the 4th column, features_batch, spatial_size = element-wise maximum,
    batch_size, batch_splits), `gt_bbox`, `gt_label` (lists), `gt_mask`, `gt_segmentation`, `batch_splits`, `augmentation`.
    Nothing leaves the tensors' device (DEVIATION: the reference moves coords_batch to the host).  Per-sample PackedMasks are
    joined into one PackedMasks of the batch; dense masks stay the reference's list."""
    ids, coords, feats, boxes, masks, labels, segs, augs, sizes = zip(*samples)
    coords_batch = torch.cat([torch.nn.functional.pad(c, (0, 1), value=i) for i, c in enumerate(coords)])
    batch_splits = [len(c) for c in coords]
    spatial_size = torch.stack([torch.as_tensor(s) for s in sizes]).max(0).values
    data = (coords_batch, torch.cat(feats), spatial_size, len(ids), batch_splits)
    gt_mask = join_packed_masks(masks) if all(isinstance(mk, PackedMasks) for mk in masks) else masks
    return dict(id=ids, data=data, gt_bbox=boxes, gt_label=labels, gt_mask=gt_mask, gt_segmentation=torch.cat(segs),
                batch_splits=batch_splits, augmentation=augs)
