"""CPU: the torch restatement of the dense RoiAlign and of the dense class branch (tests/roialign_restate.py, written from the
specification) meets every fixture the reference's own code produced (tests/golden/make_roialign_golden.py), and the dense
class branch's checkpoint key map covers exactly the reference's keys and shapes.

Bars.  bbox_tensor: bit-equal (three IEEE operations in the reference's order).  Output: max|got - ref| <= 2e-6 max|F| -- indices
and weights are the same IEEE operations in the same order, hence bit-equal; each side then rounds at most 10 times (2 for the
weight product, 1 multiply, 7 adds) on a convex combination: 10 * 2^-24 = 6e-7 per side.  Gradient: relative L2 <= 2e-5, the
project's fp32 gradient bar (the generator asserts the reference's own fp32-vs-float64 figure <= 5e-6)."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import roialign_restate as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
CASES = ["mixed", "small8", "aniso", "whole40", "empty"]
OUT_BAR, GRAD_BAR = 2e-6, 2e-5


def test_every_fixture_is_listed_and_small():
    names = sorted(os.path.basename(p)[len("roialign_"):-4] for p in glob.glob(os.path.join(GOLDEN, "roialign_*.npz")))
    assert names == sorted(CASES)
    for p in glob.glob(os.path.join(GOLDEN, "roialign_*.npz")) + glob.glob(os.path.join(GOLDEN, "dense_class_*")):
        assert os.path.getsize(p) <= 100_000, p


@pytest.mark.parametrize("name", CASES)
def test_restatement_meets_the_fixture(name):
    z = R.load_case(os.path.join(GOLDEN, f"roialign_{name}.npz"))
    assert float(z["ref_grad_rel_l2"]) <= 5e-6
    boxes = [torch.from_numpy(b) for b in z["bbox_batch"]]
    bbox, counts, sample = R.transform_boxes(boxes, z["_size"], z["_stride"], True)
    assert counts == [int(v) for v in z["counts"]]
    assert bbox.numpy().tobytes() == z["bbox_tensor"].tobytes()
    vol = torch.from_numpy(z["volume"]).requires_grad_()
    out = R.roialign(vol, bbox, sample, z["_extract"])
    c = z["_c"]
    assert tuple(out.shape) == (bbox.shape[0],) + z["_extract"] + (c,)
    rows = out.detach().numpy().reshape(-1, c)
    so, sg = int(z["out_step"]), int(z["grad_step"])
    if rows.shape[0]:
        err = np.abs(rows[::so] - z["out_rows"]).max() / float(z["vol_absmax"])
        print(f"{name}: out max err / max|F| {err:.2e}")
        assert err <= OUT_BAR
        assert abs(np.sqrt((rows.astype(np.float64) ** 2).sum()) - float(z["out_norm"])) <= 1e-5 * float(z["out_norm"])
        out.backward(torch.from_numpy(z["dout"]))
        grad = vol.grad.numpy().reshape(-1, c)
    else:
        grad = np.zeros((int(z["n_grad_rows"]), c), np.float32)
    zero = np.unpackbits(z["grad_zero_rows"])[:grad.shape[0]].astype(bool)
    assert (grad[zero] == 0).all()
    if rows.shape[0]:
        rel = R.rel_l2(grad[::sg], z["grad_rows"])
        print(f"{name}: grad rel L2 {rel:.2e}")
        assert rel <= GRAD_BAR
        assert abs(np.sqrt((grad.astype(np.float64) ** 2).sum()) - float(z["grad_norm"])) <= 1e-4 * float(z["grad_norm"])
    else:
        assert (z["grad_rows"] == 0).all()


def test_fixture_geometry_is_what_the_cases_promise():
    z = R.load_case(os.path.join(GOLDEN, "roialign_mixed.npz"))
    t = z["bbox_tensor"]
    assert [int(v) for v in z["counts"]] == [4, 0, 3]
    assert (t[1, 0] == 0).all() and (t[1, 1] == np.array(z["_size"]) - 1).all()            # clipped to the whole volume
    assert (t[2] == np.round(t[2])).all()                                                   # integer corners
    lo, hi, w = R.axis_samples(torch.from_numpy(t[2, 0]), torch.from_numpy(t[2, 1]), 16)
    assert torch.equal(lo, hi) and (w == 0).all()                                          # weights exactly 0, floor = ceil
    assert (np.floor(t[3, 0]) == np.floor(t[3, 1])).all()                                   # inside one cell
    assert (t[4, 0] == t[4, 1]).all() and (t[4, 0] == np.array(z["_size"]) - 1).all()      # outside: the corner cell
    assert (t[5] == t[6]).all()
    z4 = R.load_case(os.path.join(GOLDEN, "roialign_whole40.npz"))
    zero = np.unpackbits(z4["grad_zero_rows"])[:int(z4["n_grad_rows"])].astype(bool)
    assert zero.any() and not zero.all()                                                    # cells no sample touches


def test_key_map_covers_the_reference_keys_and_shapes():
    from sparse_rcnn_amd.classhead import DenseClassBranch, dense_reference_key_map, conv3d_to_slab_weight
    keys = json.load(open(os.path.join(GOLDEN, "dense_class_keys.json")))
    small = json.load(open(os.path.join(GOLDEN, "dense_class_small.json")))
    assert small["keys"] == keys["small"] and small["n_params"] == 22645
    for kind, branch in (("small", DenseClassBranch(12, 8, 8, (8, 16), (8,), 5)), ("real", DenseClassBranch(128, 4))):
        kmap = branch.reference_key_map()
        assert kmap == dense_reference_key_map()
        assert sorted(kmap) == sorted(keys[kind])
        own = branch.named_oracle_params()
        assert sorted(kmap.values()) == sorted(own) and len(own) == len(list(branch.parameters()))
        for rk, name in kmap.items():
            shape = keys[kind][rk]
            t = torch.zeros(shape)
            got = conv3d_to_slab_weight(t).shape if len(shape) == 5 else t.shape
            assert tuple(got) == tuple(own[name].shape), (rk, name)


def test_weight_permutation_round_trips_and_loads():
    from sparse_rcnn_amd.classhead import DenseClassBranch, conv3d_to_slab_weight, slab_to_conv3d_weight
    g = torch.Generator().manual_seed(0)
    for k in (1, 2, 3):
        w = torch.randn((5, 4, k, k, k), generator=g)
        W = conv3d_to_slab_weight(w)
        assert W.shape == (k ** 3, 4, 5)
        assert torch.equal(slab_to_conv3d_weight(W, k), w)
        a, b, c = k - 1, 0, k - 1
        assert torch.equal(W[(a * k + b) * k + c], w[:, :, a, b, c].t())
    small = json.load(open(os.path.join(GOLDEN, "dense_class_small.json")))
    params = {k: torch.from_numpy(v) for k, v in R.seeded_params(small["keys"], 21).items()}
    branch = DenseClassBranch(12, 8, 8, (8, 16), (8,), 5)
    sd = {"class_network." + k: v for k, v in params.items()}
    sd["mask_network.input_conv_layer.0.0.0.weight"] = torch.zeros(1)
    assert branch.load_reference_state_dict(sd) == ([], [])
    own = branch.named_oracle_params()
    for rk, name in branch.reference_key_map().items():
        ref = params[rk]
        assert torch.equal(own[name].detach(), conv3d_to_slab_weight(ref) if ref.dim() == 5 else ref)
    with pytest.raises(KeyError):
        branch.load_reference_state_dict({k: v for k, v in sd.items() if not k.endswith("linear_layer.3.bias")})


def test_dense_branch_restatement_meets_the_fixture():
    small = json.load(open(os.path.join(GOLDEN, "dense_class_small.json")))
    z = dict(np.load(os.path.join(GOLDEN, "dense_class_small.npz")))
    seed, batch, size, c = int(z["seed"]), int(z["batch"]), tuple(int(v) for v in z["size"]), int(z["c"])
    params = R.seeded_params(small["keys"], seed)
    vol = R.seeded_volume(seed, batch, size, c)
    assert abs(R.checksum(vol, z["score_grad"], *[params[k] for k in sorted(params)]) - float(z["checksum"])) < 1e-7
    sd = {k: torch.from_numpy(v).requires_grad_() for k, v in params.items()}
    counts, o, boxes = [int(v) for v in z["counts"]], 0, []
    for n in counts:
        boxes.append(torch.from_numpy(z["boxes"][o:o + n]))
        o += n
    fm = torch.from_numpy(vol).permute(0, 4, 1, 2, 3).contiguous().requires_grad_()
    scores, bbox, got_counts = R.dense_class_forward(sd, fm, boxes, float(z["stride"]), (16, 16, 16))
    assert got_counts == counts and bbox.numpy().tobytes() == z["bbox_tensor"].tobytes()
    scale = np.abs(z["scores"]).max()
    assert np.abs(scores.detach().numpy() - z["scores"]).max() <= 1e-4 * scale
    scores.backward(torch.from_numpy(z["score_grad"]))
    assert R.rel_l2(fm.grad.permute(0, 2, 3, 4, 1).reshape(-1, c).numpy(), z["volume_grad"]) <= GRAD_BAR
    step = int(z["element_step"])
    for k, p in sd.items():
        g = p.grad.numpy().reshape(-1)
        ref = z["grad/" + k]
        assert R.rel_l2(g if ref.size == g.size else g[::step], ref) <= GRAD_BAR, k
        assert abs(np.sqrt((g.astype(np.float64) ** 2).sum()) - float(z["grad_norm/" + k])) <= 1e-4 * float(z["grad_norm/" + k])


def test_python_surface_refuses_what_the_reference_never_builds():
    from sparse_rcnn_amd import roi
    with pytest.raises(NotImplementedError, match="wrap"):
        roi.RoiAlign((16, 16, 16), clip_boxes=False)
    with pytest.raises(NotImplementedError, match="padding"):
        roi.RoiAlign((16, 16, 16), padding=0.0, clip_boxes=True)
    assert roi.RoiAlign((16, 16, 16), clip_boxes=True, resize_boxes=8).extract_shape == (16, 16, 16)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes
    from sparse_rcnn_amd import _lib as L
    lib = L.load()
    h = L.host_i64(3)
    h[0], h[1], h[2] = 4, 4, 4
    e = L.host_i64(3)
    e[0], e[1], e[2] = 16, 16, 1
    p = ctypes.c_void_p(16)
    assert lib.scn_roialign_fwd(p, 1, h, 4, p, p, 3, e, p, p, None) == L.EINVAL          # an extract extent < 2
    e[2] = 3
    assert lib.scn_dense_maxpool_fwd(p, 3, e, 4, p, p, None) == L.EINVAL                  # an odd extent
    assert lib.scn_dense_maxpool_bwd(p, p, -1, e, 4, p, None) == L.EINVAL
    e[2] = 16
    assert lib.scn_roialign_fwd(p, 0, h, 4, p, p, 3, e, p, p, None) == L.EINVAL           # batch < 1
    assert lib.scn_roialign_fwd(None, 1, h, 4, None, None, 0, e, None, None, None) == L.OK   # no box: nothing to do
    assert lib.scn_dense_maxpool_fwd(None, 0, e, 4, None, None, None) == L.OK
