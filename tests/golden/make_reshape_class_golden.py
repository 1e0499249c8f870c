"""Generates the fixtures of the reference's RESHAPING class head (`simple_class`, scannet_config/run.py:706-710: identity input
network, RoiAlign 8^3, MaxPool3d(2), 3^3 same-convolutions, Reshaper, ReLU Linear ReLU Linear) by RUNNING the reference's own
ClassNetwork on the CPU (build container only, needs /root/reference; `import sparseconvnet` is satisfied by this repository's
package):

    python tests/golden/make_reshape_class_golden.py

  reshape_class_small.npz / .json      ClassNetwork(3, False, 12, 8, [I], [M, S(8)], linear_channels=[8], num_classes=5, cut 8^3)
                     in eval mode, parameters drawn from a seed in sorted-key order (tests/roialign_restate.py seeded_params), volume
                     (2; 6, 5, 4; 12), 3 + 2 boxes: key / shape list and repr (.json), class scores, the volume gradient and every
                     parameter gradient (every k-th element plus the norm for the large ones) of a seeded score gradient.
  reshape_class_two_same.npz / .json   the same for [M, S(None), S(4)]: two same-convolutions, no ReLU between them.
  reshape_class_keys.json              key / shape lists of the small shape and of the real one (128 -> 8, 512 -> 64 -> 18).

The reference's Reshaper calls `view` on the Conv3d's output, which the CPU convolution here returns non-contiguous: a forward
hook on output_conv_layer makes it contiguous, the reference's code is not touched.  Every network also runs in float64; the
reference's own fp32 gradients are asserted within 5e-6 relative L2 of it.  Only inputs and outputs are stored.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

GRAD_ELEMENT_STEP = 7


def main():
    sys.path.insert(0, "/root/reference")
    import sparse_rcnn_amd
    sys.modules["sparseconvnet"] = sparse_rcnn_amd
    from ndsis.modules.model import ClassNetwork, FeatureLevelDescriptor as FLD
    import roialign_restate as R

    def network(fc, same, lin, k):
        inp = [FLD(type='I')]
        outd = [FLD(type='M', params={'stride': 2})] + [FLD(type='S', channels=ch) for ch in same]
        cn = ClassNetwork(3, False, fc, 8, inp, outd, linear_channels=lin, num_classes=k, raw_scene=False,
                          cut_shape=(8, 8, 8), pooling_function_or_none=None, relu_after_pooling=True,
                          selection_tuple=(32, 0, True), positive_threshold=0.1, negative_threshold=0).eval()
        cn.output_conv_layer.register_forward_hook(lambda m, i, o: o.contiguous())
        return cn

    rng = np.random.default_rng(5)

    def rand_boxes(n, scene):
        a = rng.uniform(-0.1, 0.9, (n, 3)) * np.asarray(scene)
        e = rng.uniform(0.1, 0.8, (n, 3)) * np.asarray(scene)
        return np.stack([a, a + e], 1).astype(np.float32)

    def fixture(name, same, seed):
        cn = network(12, same, [8], 5)
        shapes = {k: list(v.shape) for k, v in cn.state_dict().items()}
        params = R.seeded_params(shapes, seed)
        cn.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        batch, size, c = 2, (6, 5, 4), 12
        vol = R.seeded_volume(seed, batch, size, c)
        bbox_batch = [rand_boxes(3, (48, 40, 32)), rand_boxes(2, (48, 40, 32))]
        boxes = [torch.from_numpy(b) for b in bbox_batch]
        fm = torch.from_numpy(vol).permute(0, 4, 1, 2, 3).contiguous().requires_grad_()
        scores, selection, _ = cn(fm, boxes, None)
        gs = np.random.default_rng(seed + 1).standard_normal(tuple(scores.shape)).astype(np.float32)
        scores.backward(torch.from_numpy(gs))
        # the reference in float64: how far its own fp32 gradients are from the exact ones
        cn64 = network(12, same, [8], 5).double()
        cn64.load_state_dict({k: torch.from_numpy(v).double() for k, v in params.items()})
        fm64 = torch.from_numpy(vol.astype(np.float64)).permute(0, 4, 1, 2, 3).contiguous().requires_grad_()
        scores64, _, _ = cn64(fm64, [b.double() for b in boxes], None)
        scores64.backward(torch.from_numpy(gs).double())
        own = {"volume": R.rel_l2(fm.grad.numpy(), fm64.grad.numpy())}
        g64 = dict(cn64.named_parameters())
        for k, p in cn.named_parameters():
            own[k] = R.rel_l2(p.grad.numpy(), g64[k].grad.numpy())
        assert max(own.values()) <= 5e-6, (name, own)
        z = dict(seed=np.array(seed), batch=np.array(batch), size=np.array(size), c=np.array(c), stride=np.array(8.0),
                 boxes=np.concatenate(bbox_batch), counts=np.array([len(b) for b in bbox_batch], np.int64),
                 checksum=np.array(R.checksum(vol, gs, *[params[k] for k in sorted(params)])),
                 bbox_tensor=selection[0].numpy(), scores=scores.detach().numpy(), score_grad=gs,
                 volume_grad=fm.grad.permute(0, 2, 3, 4, 1).contiguous().numpy().reshape(-1, c),
                 element_step=np.array(GRAD_ELEMENT_STEP), ref_grad_rel_l2=np.array(max(own.values())))
        for k, p in cn.named_parameters():
            g = p.grad.numpy().reshape(-1)
            z["grad_norm/" + k] = np.array(np.sqrt((g.astype(np.float64) ** 2).sum()))
            z["grad/" + k] = g if g.size <= 600 else g[::GRAD_ELEMENT_STEP]
        path = os.path.join(HERE, f"reshape_class_{name}.npz")
        np.savez_compressed(path, **z)
        assert os.path.getsize(path) <= 100_000, path
        with open(os.path.join(HERE, f"reshape_class_{name}.json"), "w") as f:
            json.dump(dict(n_params=int(sum(v.numel() for v in cn.state_dict().values())), keys=shapes, repr=repr(cn),
                           same_channels=[None if ch is None else int(ch) for ch in same]), f, indent=0, sort_keys=True)
        print(f"reshape_class_{name}: R {scores.shape[0]}, scores absmax {float(scores.detach().abs().max()):.3g}, reference fp32 vs fp64 "
              f"gradients: worst rel L2 {max(own.values()):.2e}; {os.path.getsize(path)} bytes")
        return shapes

    small = fixture("small", (8,), 31)
    fixture("two_same", (None, 4), 32)
    real = network(128, (8,), [64], 18)
    with open(os.path.join(HERE, "reshape_class_keys.json"), "w") as f:
        json.dump(dict(small=small, real={k: list(v.shape) for k, v in real.state_dict().items()}), f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
