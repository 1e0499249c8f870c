"""Torch restatement of the dense RoiAlign and of the dense class branch, written from the specification, and the
seeded inputs the roialign_* / dense_class_* fixtures were generated from (tests/golden/make_roialign_golden.py).

Per axis, with e samples between `start` and `stop` (cells, already transformed and clipped), every operation rounded once:
    step = (stop - start) / (e - 1);  c_i = min(i * step + start, stop);  lo = floor(c_i);  hi = ceil(c_i);  w = c_i - lo
sample i reads cell lo with weight 1 - w and cell hi with weight w; a corner's weight is (wx * wy) * wz and the output is the sum
over the 8 corners of F[corner] * weight.  Works on CPU and device tensors, fp32 or fp64; autograd gives the gradient.
"""
import numpy as np
import torch
import torch.nn.functional as TF


def transform_boxes(bbox_batch, size, resize=None, clip=True):
    """-> (bbox_tensor fp32 [R, 2, 3], counts, sample_of_box int64 [R]): / resize, + (-0.5), min(., size - 1).clamp(min=0)."""
    counts = [len(b) for b in bbox_batch]
    t = torch.cat([b.reshape(-1, 2, 3).float() for b in bbox_batch]) if sum(counts) else torch.zeros((0, 2, 3))
    if resize is not None:
        t = t / t.new_tensor(resize)
    t = t + t.new_tensor(-0.5)
    if clip:
        t = torch.min(t, t.new_tensor([float(int(s) - 1) for s in size])).clamp(min=0)
    sample = torch.tensor([s for s, c in enumerate(counts) for _ in range(c)], dtype=torch.long)
    return t, counts, sample


def axis_samples(start, stop, e):
    """start, stop [R] -> (lo int64 [R, e], hi int64 [R, e], w [R, e])."""
    step = (stop - start) / float(e - 1)
    i = torch.arange(e, dtype=start.dtype, device=start.device)
    c = torch.min(i[None, :] * step[:, None] + start[:, None], stop[:, None])
    lo, hi = c.floor(), c.ceil()
    return lo.long(), hi.long(), c - lo


def roialign(volume, boxes, sample_of_box, extract):
    """volume [B, X, Y, Z, C] channels-last, boxes [R, 2, 3], sample_of_box [R] -> [R, ex, ey, ez, C]."""
    r = boxes.shape[0]
    if r == 0:
        return volume.new_zeros((0,) + tuple(int(e) for e in extract) + (volume.shape[-1],))
    boxes = boxes.to(volume.dtype)
    axes = [axis_samples(boxes[:, 0, d], boxes[:, 1, d], int(extract[d])) for d in range(3)]
    shapes = [(r, -1, 1, 1), (r, 1, -1, 1), (r, 1, 1, -1)]
    b = sample_of_box.to(volume.device).long().view(r, 1, 1, 1)
    out = None
    for a in range(2):
        for bb in range(2):
            for cc in range(2):
                idx, wts = [], []
                for d, corner in enumerate((a, bb, cc)):
                    lo, hi, w = axes[d]
                    idx.append((hi if corner else lo).view(shapes[d]))
                    wts.append((w if corner else 1 - w).view(shapes[d]))
                weight = (wts[0] * wts[1]) * wts[2]
                term = volume[b, idx[0], idx[1], idx[2]] * weight[..., None]
                out = term if out is None else out + term
    return out


def dense_class_forward(sd, volume_ncxyz, bbox_batch, stride, cut_shape, n_levels=2, num_units=1):
    """The reference's dense ClassNetwork in eval mode from its state dict `sd` (its own keys, nn.Conv3d / nn.Linear layouts):
    1^3 conv + units on the volume, RoiAlign, max pool 2, [2^3/2 conv + units] x n_levels, mean, ReLU Linear ReLU Linear.
    -> (class scores [R, classes], bbox_tensor, counts)."""
    def unit(x, prefix):
        h = TF.conv3d(TF.relu(x), sd[prefix + "inner_block.1.weight"], sd[prefix + "inner_block.1.bias"], padding=1)
        h = TF.conv3d(TF.relu(h), sd[prefix + "inner_block.3.weight"], sd[prefix + "inner_block.3.bias"], padding=1)
        return x + h

    x = TF.conv3d(volume_ncxyz, sd["input_conv_layer.0.0.0.weight"], sd["input_conv_layer.0.0.0.bias"])
    for u in range(num_units):
        x = unit(x, f"input_conv_layer.0.1.{u}.")
    size = x.shape[2:]
    bbox_tensor, counts, sample = transform_boxes(bbox_batch, size, stride, True)
    cut = roialign(x.permute(0, 2, 3, 4, 1), bbox_tensor.to(x.device), sample, cut_shape).permute(0, 4, 1, 2, 3)
    x = TF.max_pool3d(cut, 2)
    for l in range(1, n_levels + 1):
        x = TF.conv3d(x, sd[f"output_conv_layer.{l}.0.0.weight"], sd[f"output_conv_layer.{l}.0.0.bias"], stride=2)
        for u in range(num_units):
            x = unit(x, f"output_conv_layer.{l}.1.{u}.")
    x = x.mean(dim=(2, 3, 4))
    x = TF.linear(TF.relu(x), sd["linear_layer.1.weight"], sd["linear_layer.1.bias"])
    x = TF.linear(TF.relu(x), sd["linear_layer.3.weight"], sd["linear_layer.3.bias"])
    return x, bbox_tensor, counts


# ---- the fixtures' seeded inputs (the generator and the tests build the same arrays) -------------------------------------------
def seeded_volume(seed, batch, size, c):
    """fp32 [B, X, Y, Z, C] channels-last, N(0, 1)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((batch,) + tuple(int(s) for s in size) + (c,)).astype(np.float32)


def seeded_dout(seed, r, extract, c):
    rng = np.random.default_rng(seed + 7919)
    return rng.standard_normal((r,) + tuple(int(e) for e in extract) + (c,)).astype(np.float32)


def seeded_params(shapes, seed):
    """{key: shape} -> {key: fp32 array}, drawn in sorted-key order: weights N(0, 1 / fan_in), biases N(0, 0.1^2)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in sorted(shapes):
        shape = tuple(int(v) for v in shapes[k])
        scale = 0.1 if len(shape) == 1 else 1.0 / np.sqrt(max(1, int(np.prod(shape[1:]))))
        out[k] = (rng.standard_normal(shape) * scale).astype(np.float32)
    return out


def checksum(*arrays):
    return float(sum(np.asarray(a, dtype=np.float64).sum() for a in arrays))


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((got - ref) ** 2).sum()) / max(np.sqrt((ref ** 2).sum()), 1e-300))


def load_case(path):
    """A roialign_*.npz fixture with its inputs regenerated -> dict (numpy arrays; boxes as a list per sample)."""
    z = dict(np.load(path))
    batch, size, c = int(z["batch"]), tuple(int(v) for v in z["size"]), int(z["c"])
    extract = tuple(int(v) for v in z["extract"])
    z["volume"] = seeded_volume(int(z["seed"]), batch, size, c)
    r = int(z["bbox_tensor"].shape[0])
    z["dout"] = seeded_dout(int(z["seed"]), r, extract, c)
    assert abs(checksum(z["volume"], z["dout"]) - float(z["checksum"])) <= 1e-9 * max(1.0, abs(float(z["checksum"])))
    counts, o, boxes = [int(v) for v in z["counts"]], 0, []
    for n in counts:
        boxes.append(z["boxes"][o:o + n])
        o += n
    z["bbox_batch"] = boxes
    z["_size"], z["_extract"], z["_batch"], z["_c"], z["_stride"] = size, extract, batch, c, float(z["stride"])
    return z
