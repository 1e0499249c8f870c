"""Training batches from stored scene samples, on the device.

`convert_sample` is ndsis/data/sparse_augmentation.py ``convert_sample`` (:250-313) and `collate` is ndsis/data/data.py
``collate_fn`` (:88-115).  The coordinate part is `voxelize.augment_coords` (scn_vox_*); this module adds what makes the batch
a supervised one -- the feature tensor, the instances that survive the cut-out with their boxes, point masks and labels, the
per-point segmentation labels, the rounded spatial size -- on scn_sample_stats / scn_sample_pack (csrc/scn_sample.hip).

Every random number of the reference is an input (`Draws`).  `draw_augmentation` / `random_cut_start` draw them on the host
with torch's CPU generator, by the reference's calls in the reference's order, so one ``torch.manual_seed`` gives the
reference's values; `convert_sample(..., draws=None)` calls them itself at the points where the reference draws.

`PhiloxDraws` is the other source: a conversion whose every random number is a function of (seed, sample counter) -- the counter-
based generator of csrc/scn_rng.h (Philox4x32-10).  The nine host values come from `philox_normals` / `philox_words` here; the
random cut-out's start is ONE launch (scn_sample_cut_start) and one 32-byte read; the per-point noise is drawn inside the pack
kernel (scn_sample_pack_drawn) and never exists as a tensor unless `augmentation['color_shift'].tensor()` asks for it.  It does
not reproduce ``torch.manual_seed``'s values: the reference's fixtures pin the host-generator path, and the tests pin this path
to that one.

Host waits of one `convert_sample`: the kept-row count (augment_coords' own) and ONE copy of the (I + 1) x 8 instance table,
queued before that count is waited for.  The random cut-out adds the three small reads of `random_cut_start` -- with a
`PhiloxDraws` one read of 32 bytes, and no noise is copied to the device.
DEVIATION: ``augmentation['remaining_points']`` stays on the device (the reference copies N bools to the host per sample).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from .loss import PackedMasks
from .voxelize import _augment_coords, _f32xn, _i32x3

__all__ = ["Draws", "PhiloxDraws", "draw_augmentation", "random_cut_start", "convert_sample", "collate", "join_packed_masks",
           "philox_words", "philox_normals"]


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


def _distortion_matrix(dtype, coord_noise_sigma, theta, mirror, normals=None, mirror_bit=None, uniform=None, pick=None):
    """get_coord_distortion_matrix (sparse_augmentation.py:9-38): randn(3,3), then randint(0,2) if mirror is None, then rand()
    if theta is None (multinomial if theta is a list).  Each draw can be handed in instead (`PhiloxDraws`): `normals` fp32
    [3,3], `mirror_bit` 0 / 1, `uniform` in (0, 1), `pick(n)` -> an index below n; a None is drawn from torch's generator."""
    m = torch.eye(3, dtype=dtype) + (torch.randn((3, 3), dtype=dtype) if normals is None else normals) * coord_noise_sigma
    if mirror is None:
        m[0, 0] *= (torch.randint(0, 2, ()) if mirror_bit is None else mirror_bit) * 2 - 1
    else:
        m[0, 0] *= -1 if mirror else 1
    if theta is None:
        angle = (torch.rand((), dtype=dtype) if uniform is None else torch.tensor(uniform, dtype=dtype)) * 2 * math.pi
    else:
        angle = torch.tensor(theta, dtype=dtype)
        if angle.numel() > 1:
            angle = angle[torch.ones_like(angle).multinomial(1)[0] if pick is None else pick(angle.numel())]
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


# ---- the counter-based generator (csrc/scn_rng.h), restated for the host's handful of values ----

_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox_words(seed, counter, stream, index):
    """Philox4x32-10 with key = (seed lo32, seed hi32) and counter = (index, stream, counter lo32, counter hi32): the draw
    scn_rng.h's scn_rng_draw makes.  seed / counter: Python integers below 2^64; stream / index: integers or integer arrays
    (broadcast).  -> numpy uint32 [..., 4]."""
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    index, stream = np.broadcast_arrays(np.asarray(index, dtype=np.uint64), np.asarray(stream, dtype=np.uint64))
    c = [index & _MASK32, stream & _MASK32, np.full(index.shape, counter & 0xFFFFFFFF, np.uint64),
         np.full(index.shape, counter >> 32, np.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c[0], np.uint64(_PHILOX_M1) * c[2]        # 32 x 32 -> 64: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK32]
        k0, k1 = (k0 + _PHILOX_W0) & 0xFFFFFFFF, (k1 + _PHILOX_W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def _philox_uniform(words):
    """u(w) = ((w >> 9) + 0.5) * 2^-23 in float64 (the same value as the fp32 form: it is exact in both)."""
    return ((words >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def philox_normals(seed, counter, stream, index):
    """The three normals of each draw -- z0 = r0 cos(2 pi u1), z1 = r0 sin(2 pi u1), z2 = r1 cos(2 pi u3), r0 = sqrt(-2 ln u0),
    r1 = sqrt(-2 ln u2) -- computed in float64 and cast: numpy fp32 [..., 3].  For the host's few values; the device's fp32
    evaluation of the same words (scn_philox_fill) agrees to a few ulp, not to the bit."""
    u = _philox_uniform(philox_words(seed, counter, stream, index))
    r0, r1 = np.sqrt(-2 * np.log(u[..., 0])), np.sqrt(-2 * np.log(u[..., 2]))
    z = np.stack([r0 * np.cos(2 * np.pi * u[..., 1]), r0 * np.sin(2 * np.pi * u[..., 1]), r1 * np.cos(2 * np.pi * u[..., 3])], -1)
    return z.astype(np.float32)


class _LazyNoise:
    """`augmentation['color_shift']` / `['normals_shift']` of a `PhiloxDraws` conversion: the noise the pack kernel added, as a
    recipe.  `.tensor()` materialises it on the device (scn_philox_fill): fp32 [3] (common) or [M, 3]."""

    def __init__(self, draws, which, m, sigma, common, device):
        self.draws, self.which, self.m, self.sigma, self.common, self.device = draws, which, m, sigma, common, device

    def tensor(self):
        return self.draws.noise_tensor(self.which, self.m, self.sigma, self.common, device=self.device)


class PhiloxDraws(Draws):
    """The draws of one conversion as a function of (seed, counter): one seed per run, counter = the global index of the sample
    (INTEGRATION.md), so no two conversions share a value whatever rank or step makes them.

    Host part, stream 0, through `_distortion_matrix`'s arithmetic: the normals of indices 0 .. 2 are the rows of the 3 x 3 that
    coord_noise_sigma scales; of index 3, the low bit of word 0 is the mirror (1 = mirrored) and word 1 the angle (u * 2 pi) or
    the pick from a list of angles ((w * len) >> 32); the uniforms of words 0 .. 2 of index 4 are the sub-pixel offset.  Fixed
    theta / mirror / sub_pixel_offset pass through, as in `draw_augmentation`.  `start_positions` may be set by hand (a given
    start); left None, `convert_sample` fills it from scn_sample_cut_start, together with `cut_order` / `cut_alive` /
    `cut_dims`.  The noise is never stored here: `convert_sample` draws it inside the pack kernel."""

    def __init__(self, seed, counter, *, coord_noise_sigma=0, theta=None, mirror=None, sub_pixel_offset=None):
        self.seed, self.counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
        z = torch.from_numpy(philox_normals(self.seed, self.counter, L.RNG_HOST, np.arange(3)))
        w = philox_words(self.seed, self.counter, L.RNG_HOST, np.arange(3, 5))
        ortho = _distortion_matrix(torch.float32, coord_noise_sigma, theta, mirror, normals=z, mirror_bit=int(w[0, 0] & 1),
                                   uniform=float(_philox_uniform(w[0, 1])), pick=lambda n: (int(w[0, 1]) * n) >> 32)
        if sub_pixel_offset is None:
            sub_pixel_offset = torch.from_numpy(_philox_uniform(w[1, :3]).astype(np.float32))
        super().__init__(ortho, sub_pixel_offset)
        self.cut_order = self.cut_alive = self.cut_dims = None

    def cut_start(self, discrete, size, border):
        """random_cut_out's start positions for the device voxels `discrete` int32 [N, 3]: one launch, one 32-byte read.
        Fills start_positions (int64 [3], host), cut_order, cut_alive and cut_dims (scn_sample_cut_start's out8)."""
        out8 = torch.empty(8, dtype=torch.int32, device=discrete.device)
        L.check(L.lib().scn_sample_cut_start(L.ptr(discrete), discrete.shape[0], _i32x3(size), _i32x3(border), self.seed,
                                             self.counter, L.ptr(out8), L.stream()))
        host = out8.cpu()                                        # the one read of the random cut-out
        self.start_positions = host[:3].to(torch.int64)
        self.cut_order, self.cut_alive, self.cut_dims = host[3:6].tolist(), int(host[6]), int(host[7])
        return self.start_positions

    def noise_tensor(self, which, m, sigma, common, device=None):
        """The noise `convert_sample` adds for `which` = 'color' | 'normal', materialised on the device by scn_philox_fill:
        fp32 [3] (common) or [m, 3] (kept-row order) = sigma * z, bit for bit what the pack kernel adds."""
        stream = {("color", False): L.RNG_COLOR, ("normal", False): L.RNG_NORMAL, ("color", True): L.RNG_COLOR_COMMON,
                  ("normal", True): L.RNG_NORMAL_COMMON}[(which, bool(common))]
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        n = 1 if common else int(m)
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
        L.check(L.lib().scn_philox_fill(self.seed, self.counter, stream, 0, n, 1, float(sigma), L.ptr(out), L.stream()))
        return out[0] if common else out


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
    theta / mirror / sub_pixel_offset here.  With a `Draws`, those four keywords are not read.  A `PhiloxDraws`: nothing is
    drawn on the host -- the random cut-out's start comes from scn_sample_cut_start (one launch, one small read; written back
    to `draws.start_positions`), the noise is drawn inside scn_sample_pack_drawn, and `augmentation['color_shift']` /
    `['normals_shift']` are objects whose `.tensor()` materialises what was added (without noise: the zero-dim zero, as ever).
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
    philox = isinstance(draws, PhiloxDraws)

    start_positions = None
    if spatial_size is not None and shift is None:
        if draws.start_positions is not None:
            start_positions = draws.start_positions
        else:
            size3 = [int(s) for s in torch.as_tensor(spatial_size).expand(3).tolist()]
            border = [0, 0, 0] if max_empty_border_size_divisor is None else [s // max_empty_border_size_divisor for s in size3]

            def start_positions(discrete):
                if philox:
                    return draws.cut_start(discrete, size3, border)
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

    if not philox:
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
    if philox:                                               # the noise is drawn inside the kernel: no randn, no copy
        csig = float(color_noise_sigma) if (use_color and color_noise_sigma) else 0.0
        nsig = float(normal_noise_sigma) if (use_normal and normal_noise_sigma) else 0.0
        cn = _LazyNoise(draws, "color", m, csig, bool(common_color_noise), dev) if csig else None
        nn_ = _LazyNoise(draws, "normal", m, nsig, bool(common_normal_noise), dev) if nsig else None
        L.check(lib.scn_sample_pack_drawn(
            L.ptr(rows), m, L.ptr(colors), L.ptr(normals), L.ptr(instance_ids), n_inst, _f32xn(draws.almost_orthonormal, 9),
            draws.seed, draws.counter, csig, int(bool(common_color_noise)), nsig, int(bool(common_normal_noise)),
            int(bool(use_color)), int(bool(use_ones)), int(bool(use_normal)), L.ptr(features) if c else 0,
            L.ptr(seg_table_dev), L.ptr(seg), L.ptr(slot_dev), g, L.ptr(words), L.stream()))
    else:
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
