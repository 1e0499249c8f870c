"""Without a GPU: the restatement the bf16 dense class branch is tested against (tests/dense_class_bf16_restate.py) reproduces the
reference's own fixture with identity hooks; the two bounds of tests/test_gpu_roialign_bf16.py hold for an fp32 evaluation of
the restated RoiAlign on bf16 inputs whose result is rounded once -- what the bf16 entry points are specified to compute;
DenseClassBranch refuses bf16 storage at widths that have no 16-byte lanes; the header declares the four calls."""
import json
import os
import re

import numpy as np
import pytest
import torch

import dense_class_bf16_restate as D
import roialign_restate as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)


def _boxes(z):
    counts, o, boxes = [int(v) for v in z["counts"]], 0, []
    for n in counts:
        boxes.append(torch.from_numpy(z["boxes"][o:o + n]))
        o += n
    return boxes


def test_identity_hooks_reproduce_the_reference_fixture():
    small = json.load(open(os.path.join(GOLDEN, "dense_class_small.json")))
    z = dict(np.load(os.path.join(GOLDEN, "dense_class_small.npz")))
    seed, batch, size, c = int(z["seed"]), int(z["batch"]), tuple(int(v) for v in z["size"]), int(z["c"])
    sd = {k: torch.from_numpy(v) for k, v in R.seeded_params(small["keys"], seed).items()}
    vol = torch.from_numpy(R.seeded_volume(seed, batch, size, c)).permute(0, 4, 1, 2, 3)
    scores, bbox, counts = D.dense_class_forward(sd, vol, _boxes(z), float(z["stride"]), (16, 16, 16))
    assert counts == [int(v) for v in z["counts"]] and bbox.numpy().tobytes() == z["bbox_tensor"].tobytes()
    scale = float(np.abs(z["scores"]).max())
    err = float(np.abs(scores.numpy() - z["scores"]).max())
    print(f"[restatement, identity hooks] scores max err {err:.2e} (scale {scale:.3g})")
    assert err <= 1e-4 * scale
    # the hooks are live: bf16 roundings move the scores
    rounded, _, _ = D.dense_class_forward(sd, D.bf16_round(vol), _boxes(z), float(z["stride"]), (16, 16, 16), q=D.bf16_round,
                                          wq=D.bf16_round)
    moved = float((rounded - scores).abs().max())
    print(f"[restatement, bf16 hooks] scores moved by {moved:.2e}")
    assert moved > 0


@pytest.mark.parametrize("c", D.WIDTHS)
@pytest.mark.parametrize("name", D.GEOMETRIES)
def test_bf16_bounds_hold_for_the_once_rounded_fp32_restatement(name, c):
    z = R.load_case(os.path.join(GOLDEN, f"roialign_{name}.npz"))
    vol, boxes, sample, dout = D.bf16_case(z, c)
    a = vol.clone().requires_grad_()
    out = R.roialign(a, boxes, sample, z["_extract"])                 # fp32 arithmetic on the widened inputs
    out.backward(dout)
    ref_out, ref_grad = D.float64_reference(name, z, c)
    slack = D.forward_slack(D.bf16_round(out.detach()), ref_out, float(vol.abs().max()))
    rel = D.rel_l2(D.bf16_round(a.grad).numpy(), ref_grad.numpy())
    print(f"[bf16 bounds] {name} C={c}: forward worst slack {slack:.2e} (<= 0), backward relative L2 {rel:.2e} (<= {D.GRAD_BAR:.2e})")
    assert slack <= 0
    assert rel <= D.GRAD_BAR


def test_dense_class_branch_refuses_widths_without_lanes():
    from sparse_rcnn_amd.classhead import DenseClassBranch
    with pytest.raises(ValueError, match="multiple of 8"):
        DenseClassBranch(12, 8, storage=torch.bfloat16)
    with pytest.raises(ValueError, match="multiple of 8"):
        DenseClassBranch(16, 8, 8, (8, 12), (8,), 5, storage=torch.bfloat16)
    with pytest.raises(ValueError):
        DenseClassBranch(16, 8, storage=torch.float16)
    assert DenseClassBranch(12, 8, 8, (8, 16), (8,), 5).storage is torch.float32         # the default: nothing changes
    assert DenseClassBranch(16, 8, 8, (8, 16), (8,), 5, storage=torch.bfloat16).storage is torch.bfloat16


def test_header_and_binding_declare_the_four_calls():
    text = open(os.path.join(ROOT, "include", "scn_mi355x.h")).read()
    from sparse_rcnn_amd import _lib as L
    for name in ("scn_roialign_fwd_bf16", "scn_roialign_bwd_bf16", "scn_dense_maxpool_fwd_bf16", "scn_dense_maxpool_bwd_bf16"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl, name
        assert "uint16_t*" in decl.group(1) and "float* F" not in decl.group(1)
        twin = re.search(r"\bint " + name[:-5] + r"\(([^;]*)\);", text)
        assert decl.group(1).count(",") == twin.group(1).count(",")                     # the fp32 form's arguments
        assert name in L.EXPORTS and L._SIGS[name] == L._SIGS[name[:-5]]
    assert re.search(r"#define SCN_ABI_VERSION 5\b", text)


def test_raw_calls_refuse_rows_without_lanes_before_any_launch():
    """The refusals need no device: a width that is no multiple of 8, or a pointer off a 16-byte boundary, returns SCN_EINVAL."""
    from sparse_rcnn_amd import _lib as L
    lib = L.load()
    size, extract = (L.i64 * 3)(6, 5, 4), (L.i64 * 3)(8, 8, 8)
    for c, ptr in ((12, 4096), (8, 4096 + 2)):
        assert lib.scn_roialign_fwd_bf16(ptr, 2, size, c, 4096, 4096, 5, extract, 4096, 4096, None) == L.EINVAL
        assert b"bf16 rows need" in lib.scn_last_error_string()
        assert lib.scn_roialign_bwd_bf16(ptr, 4096, 4096, 5, 2, size, c, extract, 4096, None) == L.EINVAL
        assert lib.scn_dense_maxpool_fwd_bf16(ptr, 5, extract, c, 4096, 4096, None) == L.EINVAL
        assert lib.scn_dense_maxpool_bwd_bf16(ptr, 4096, 5, extract, c, 4096, None) == L.EINVAL
