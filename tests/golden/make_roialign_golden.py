"""Generates the dense RoiAlign / dense class branch fixtures by RUNNING the reference's own code on the CPU (build container
only, needs /root/reference; `import sparseconvnet` is satisfied by this repository's package):

    python tests/golden/make_roialign_golden.py

  roialign_*.npz     ndsis/modules/roi_select_dense.py RoiAlign(extract, clip_boxes=True, resize_boxes=stride) on a seeded
                     channels-last volume (tests/roialign_restate.py seeded_volume; a float64 checksum is stored): the returned
                     bbox_tensor, the output, the feature-map gradient of a seeded dOut, and the fp32-vs-float64 relative L2 of
                     the reference's own gradient (asserted <= 5e-6).  Large outputs: every k-th row plus the norm.
  dense_class_small.npz / .json   the reference's dense ClassNetwork(3, False, 12, 8, ...) in eval mode with parameters drawn from
                     a seed in sorted-key order: key / shape list and repr (.json), class scores, feature-map gradient and
                     every parameter gradient (every k-th element plus the norm for the large ones) of a seeded score gradient.
  dense_class_keys.json   key / shape lists of the small network and of the real shape (feature_channels 128, 32 / 64 / 128,
                     18 classes).
Only inputs and outputs are stored.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

OUT_BYTES_WHOLE = 24_000         # an array up to this many bytes is stored whole
GRAD_ELEMENT_STEP = 7


def rows_step(n_rows, row_bytes, budget):
    return max(1, -(-n_rows * row_bytes // budget))


def main():
    sys.path.insert(0, "/root/reference")
    import sparse_rcnn_amd
    sys.modules["sparseconvnet"] = sparse_rcnn_amd
    from ndsis.modules.roi_select_dense import RoiAlign
    from ndsis.modules.model import ClassNetwork, FeatureLevelDescriptor as FLD
    import roialign_restate as R

    def case(name, seed, batch, size, extract, stride, c, bbox_batch):
        vol = R.seeded_volume(seed, batch, size, c)
        align = RoiAlign(extract, clip_boxes=True, resize_boxes=stride)
        boxes = [torch.from_numpy(np.asarray(b, np.float32).reshape(-1, 2, 3)) for b in bbox_batch]
        r = sum(len(b) for b in boxes)
        dout = R.seeded_dout(seed, r, extract, c)
        fm = torch.from_numpy(vol).permute(0, 4, 1, 2, 3).contiguous().requires_grad_()
        out, (bbox_tensor, counts, scene_shape) = align(fm, boxes)
        assert tuple(scene_shape) == tuple(size) and list(counts) == [len(b) for b in boxes]
        go = torch.from_numpy(dout).permute(0, 4, 1, 2, 3)
        out.backward(go)
        grad = fm.grad.permute(0, 2, 3, 4, 1).contiguous().numpy().reshape(-1, c)          # slab rows
        out_rows = out.detach().permute(0, 2, 3, 4, 1).contiguous().numpy().reshape(-1, c)
        # the reference in float64 on the same (fp32) transformed boxes
        fm64 = torch.from_numpy(vol.astype(np.float64)).permute(0, 4, 1, 2, 3).contiguous().requires_grad_()
        if r:
            assoc = torch.tensor([s for s, b in enumerate(boxes) for _ in range(len(b))], dtype=torch.long)
            out64 = align.roi_align_inner(fm64, bbox_tensor.double(), assoc)
            out64.backward(go.double())
            grad64 = fm64.grad.permute(0, 2, 3, 4, 1).contiguous().numpy().reshape(-1, c)
            ref_err = R.rel_l2(grad, grad64)
            out_err = float(np.abs(out_rows - out64.detach().permute(0, 2, 3, 4, 1).numpy().reshape(-1, c)).max()
                            / np.abs(vol).max())
        else:
            grad64, ref_err, out_err = np.zeros_like(grad, dtype=np.float64), 0.0, 0.0
        assert ref_err <= 5e-6, (name, ref_err)
        so = rows_step(out_rows.shape[0], 4 * c, 36_000) if out_rows.nbytes > OUT_BYTES_WHOLE else 1
        sg = rows_step(grad.shape[0], 4 * c, 44_000) if grad.nbytes > OUT_BYTES_WHOLE else 1
        flat = np.concatenate([np.asarray(b, np.float32).reshape(-1, 2, 3) for b in bbox_batch] + [np.zeros((0, 2, 3), np.float32)])
        z = dict(seed=np.array(seed), batch=np.array(batch), size=np.array(size), extract=np.array(extract),
                 stride=np.array(float(stride)), c=np.array(c), boxes=flat, counts=np.array([len(b) for b in boxes], np.int64),
                 checksum=np.array(R.checksum(vol, dout)), bbox_tensor=bbox_tensor.numpy(),
                 out_step=np.array(so), out_rows=out_rows[::so], out_norm=np.array(np.sqrt((out_rows.astype(np.float64) ** 2).sum())),
                 grad_step=np.array(sg), grad_rows=grad[::sg], grad_norm=np.array(np.sqrt((grad.astype(np.float64) ** 2).sum())),
                 grad_zero_rows=np.packbits(~(grad64 != 0).any(axis=1)), n_grad_rows=np.array(grad.shape[0]),
                 ref_grad_rel_l2=np.array(ref_err), ref_out_err=np.array(out_err), vol_absmax=np.array(np.abs(vol).max()))
        path = os.path.join(HERE, f"roialign_{name}.npz")
        np.savez_compressed(path, **z)
        neg = float((out_rows < 0).mean()) if r else 0.0
        print(f"roialign_{name}: R {r} out rows {out_rows.shape[0]} (step {so}) grad rows {grad.shape[0]} (step {sg}), "
              f"untouched cells {int((~(grad64 != 0).any(axis=1)).sum())}, negative outputs {neg:.2f}, reference fp32 vs fp64: "
              f"grad rel L2 {ref_err:.2e}, out max err / max|F| {out_err:.2e}; {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) <= 100_000, path

    # 1: stride 8, volume 20 x 6 x 5, three samples (the middle one without a box)
    s0 = [[[13., 7., 5.], [101., 39., 30.]],                 # a general box
          [[-20., -20., -20.], [400., 400., 400.]],          # clipped on both sides to the whole volume
          [[12., 20., 12.], [132., 20., 12.]],               # transformed corners are integers: x samples 1, 2, .. 16, y = 2, z = 1
          [[21.6, 12.8, 29.6], [25.6, 16.8, 35.2]]]          # inside one cell
    s2 = [[[300., 300., 300.], [350., 350., 350.]],          # entirely outside: clips to the corner cell
          [[30., 5., 3.], [90., 40., 33.]],
          [[30., 5., 3.], [90., 40., 33.]]]                  # the same box twice
    case("mixed", 11, 3, (20, 6, 5), (16, 16, 16), 8, 12, [s0, [], s2])
    rng = np.random.default_rng(5)

    def rand_boxes(n, scene):
        a = rng.uniform(-0.1, 0.9, (n, 3)) * np.asarray(scene)
        e = rng.uniform(0.1, 0.8, (n, 3)) * np.asarray(scene)
        return np.stack([a, a + e], 1).astype(np.float32)

    case("small8", 12, 2, (6, 5, 4), (8, 8, 8), 4, 8, [rand_boxes(3, (24, 20, 16)), rand_boxes(2, (24, 20, 16))])
    case("aniso", 13, 2, (5, 7, 3), (4, 6, 2), 8, 6, [rand_boxes(2, (40, 56, 24)), rand_boxes(4, (40, 56, 24))])
    case("whole40", 14, 1, (40, 3, 3), (16, 16, 16), 8, 4, [[[[-8., -8., -8.], [400., 100., 100.]]]])
    case("empty", 15, 2, (4, 4, 4), (16, 16, 16), 8, 4, [[], []])

    # ---- the dense class network ----
    common = dict(main_path_relu=False, relu_first=True, bottleneck_divisor=0, drop_input_relu=True, make_dense=False,
                  num_units=1)

    def network(fc, cin, couts, lin, k):
        inp = [FLD(type='B', channels=cin, params={**common, 'stride': 1}, anchor_path=None)]
        outd = [FLD(type='M', channels=None, params={'stride': 2}, anchor_path=None)] + [
            FLD(type='B', channels=ch, params={**common, 'stride': 2}, anchor_path=None) for ch in couts]
        return ClassNetwork(3, False, fc, 8, inp, outd, linear_channels=lin, num_classes=k, raw_scene=False,
                            cut_shape=(16, 16, 16), pooling_function_or_none=torch.mean, relu_after_pooling=True,
                            selection_tuple=(32, 0, True), positive_threshold=0.1, negative_threshold=0).eval()

    cn = network(12, 8, (8, 16), [8], 5)
    shapes = {k: list(v.shape) for k, v in cn.state_dict().items()}
    n_params = int(sum(v.numel() for v in cn.state_dict().values()))
    assert n_params == 22645, n_params
    seed = 21
    params = R.seeded_params(shapes, seed)
    cn.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    batch, size, c = 2, (6, 5, 4), 12
    vol = R.seeded_volume(seed, batch, size, c)
    bbox_batch = [rand_boxes(3, (48, 40, 32)), rand_boxes(2, (48, 40, 32))]
    fm = torch.from_numpy(vol).permute(0, 4, 1, 2, 3).contiguous().requires_grad_()
    scores, selection, _ = cn(fm, [torch.from_numpy(b) for b in bbox_batch], None)
    gs = np.random.default_rng(seed + 1).standard_normal(tuple(scores.shape)).astype(np.float32)
    scores.backward(torch.from_numpy(gs))
    z = dict(seed=np.array(seed), batch=np.array(batch), size=np.array(size), c=np.array(c), stride=np.array(8.0),
             boxes=np.concatenate(bbox_batch), counts=np.array([len(b) for b in bbox_batch], np.int64),
             checksum=np.array(R.checksum(vol, gs, *[params[k] for k in sorted(params)])),
             bbox_tensor=selection[0].numpy(), scores=scores.detach().numpy(), score_grad=gs,
             volume_grad=fm.grad.permute(0, 2, 3, 4, 1).contiguous().numpy().reshape(-1, c),
             element_step=np.array(GRAD_ELEMENT_STEP))
    for k, p in cn.named_parameters():
        g = p.grad.numpy().reshape(-1)
        z["grad_norm/" + k] = np.array(np.sqrt((g.astype(np.float64) ** 2).sum()))
        z["grad/" + k] = g if g.size <= 600 else g[::GRAD_ELEMENT_STEP]
    path = os.path.join(HERE, "dense_class_small.npz")
    np.savez_compressed(path, **z)
    assert os.path.getsize(path) <= 100_000
    with open(os.path.join(HERE, "dense_class_small.json"), "w") as f:
        json.dump(dict(n_params=n_params, keys=shapes, repr=repr(cn)), f, indent=0, sort_keys=True)
    real = network(128, 32, (64, 128), [64], 18)
    with open(os.path.join(HERE, "dense_class_keys.json"), "w") as f:
        json.dump(dict(small=shapes, real={k: list(v.shape) for k, v in real.state_dict().items()}), f, indent=0, sort_keys=True)
    print(f"dense_class_small: R {scores.shape[0]}, scores absmax {float(scores.abs().max()):.3g}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
