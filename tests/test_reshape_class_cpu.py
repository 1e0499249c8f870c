"""CPU: the reshaping class head (classhead.ReshapeClassBranch) -- its checkpoint key map against the key lists of reference
networks, the torch restatement (tests/reshape_class_restate.py) against the fixtures the reference's own code produced
(tests/golden/make_reshape_class_golden.py), and the refusals that need no GPU.

Bar of the restatement: scores and every gradient within 1e-6 of the reference array's own scale (max |ref|).  Both sides are
fp32 torch on the CPU running the same operations; what separates them is the summation order of RoiAlign's 8 corners (the
reference adds them in another grouping), a few ulp of values of order 1."""
import json
import os

import numpy as np
import pytest
import torch

import reshape_class_restate as S

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FIXTURES = ["small", "two_same"]


def test_key_map_matches_the_reference_key_lists():
    from sparse_rcnn_amd.classhead import ReshapeClassBranch, conv3d_to_slab_weight
    keys = json.load(open(os.path.join(GOLDEN, "reshape_class_keys.json")))
    for shapes, branch in ((keys["small"], ReshapeClassBranch(12, 8, (8,), (8,), 5)),
                           (keys["real"], ReshapeClassBranch(128, 4)),
                           (json.load(open(os.path.join(GOLDEN, "reshape_class_two_same.json")))["keys"],
                            ReshapeClassBranch(12, 8, (None, 4), (8,), 5))):
        kmap, own = branch.reference_key_map(), branch.named_oracle_params()
        assert sorted(kmap) == sorted(shapes)
        assert sorted(kmap.values()) == sorted(own) and len(own) == len(list(branch.parameters()))
        for rk, name in kmap.items():
            ref = torch.zeros(shapes[rk])
            assert tuple((conv3d_to_slab_weight(ref) if ref.dim() == 5 else ref).shape) == tuple(own[name].shape), rk
    # relu_after_pooling=False: the reference's linear stack then starts with the Linear itself (start_relu=False)
    bare = ReshapeClassBranch(12, 8, (8,), (8,), 5, relu_after_pooling=False)
    assert [type(m).__name__ for m in bare.linear_layer] == ["Linear", "ReLU", "Linear"]
    assert {"linear_layer.0.weight", "linear_layer.2.bias"} <= set(bare.reference_key_map())
    real = ReshapeClassBranch(128, 4)
    assert real.linear_layer[1].in_features == 512 and real.output_conv_layer[0].nOut == 8 and real.fused


def test_loading_a_reference_state_dict_on_the_cpu():
    from sparse_rcnn_amd.classhead import ReshapeClassBranch, slab_to_conv3d_weight
    z = S.load_fixture(GOLDEN, "two_same")
    sd = {"class_network." + k: torch.from_numpy(v) for k, v in z["params"].items()}
    sd["mask_network.output_conv_layer.1.weight"] = torch.zeros(3, 3)
    branch = ReshapeClassBranch(12, 8, (None, 4), (8,), 5)
    assert branch.load_reference_state_dict(sd) == ([], [])
    own = branch.named_oracle_params()
    w = slab_to_conv3d_weight(own["same1.weight"].detach(), 3)
    assert torch.equal(w, sd["class_network.output_conv_layer.2.weight"])
    assert torch.equal(own["lin0.weight"].detach(), sd["class_network.linear_layer.1.weight"])
    del sd["class_network.linear_layer.3.bias"]
    with pytest.raises(KeyError):
        branch.load_reference_state_dict(sd)
    assert branch.load_reference_state_dict(sd, strict=False) == (["class_network.linear_layer.3.bias"], [])


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_fixture(name):
    z = S.load_fixture(GOLDEN, name)
    sd = {k: torch.from_numpy(v).requires_grad_() for k, v in z["params"].items()}
    vol = torch.from_numpy(z["volume"]).permute(0, 4, 1, 2, 3).contiguous().requires_grad_()
    scores, bbox, counts = S.reshape_class_forward(sd, vol, [torch.from_numpy(b) for b in z["bbox_batch"]], float(z["stride"]))
    assert counts == [int(v) for v in z["counts"]] and bbox.numpy().tobytes() == z["bbox_tensor"].tobytes()

    def close(got, ref, what):
        err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
        print(f"[reshape class restatement] {name} {what}: max err {err:.2e} (scale {scale:.3g})")
        assert err <= 1e-6 * scale, what

    close(scores.detach().numpy(), z["scores"], "scores")
    scores.backward(torch.from_numpy(z["score_grad"]))
    close(vol.grad.permute(0, 2, 3, 4, 1).reshape(-1, z["_c"]).numpy(), z["volume_grad"], "volume gradient")
    step = int(z["element_step"])
    for k, p in sd.items():
        g, ref = p.grad.numpy().reshape(-1), z["grad/" + k]
        close(g if g.size == ref.size else g[::step], ref, k)


def test_refusals():
    from sparse_rcnn_amd.classhead import ReshapeClassBranch
    from sparse_rcnn_amd.trainstep import SceneStep, SparseStepModel
    for cut in ((8, 7, 8), (0, 8, 8), (8, 8)):
        with pytest.raises(ValueError):
            ReshapeClassBranch(12, 8, cut_shape=cut)
    with pytest.raises(ValueError):
        ReshapeClassBranch(12, 8, same_channels=())
    kw = dict(rpn_loss=True, class_loss=True)
    with pytest.raises(ValueError, match="dense_class"):
        SceneStep("cfg3-rpn", simple_class=True, **kw)
    with pytest.raises(ValueError, match="class_storage"):
        SceneStep("cfg3-rpn", dtype="bf16", dense_class=True, simple_class=True, class_storage="bf16", **kw)
    with pytest.raises(ValueError, match="dense_class"):
        SparseStepModel((16, 32), False, False, "stand-in", with_class=True, simple_class=True)
