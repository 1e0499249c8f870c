"""No GPU: the bf16 stand-alone ReLU's entry points are exported, declared and counted consistently, and MultiLevelRpn takes the
up-sampling heads together with a bf16-stored stack (tests/test_gpu_relu_bf16.py runs them)."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scn_relu_fwd_bf16", "scn_relu_bwd_bf16")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_entry_points_are_exported_and_declared():
    import sparse_rcnn_amd as scn
    from sparse_rcnn_amd import _lib as L
    header = _read("include", "scn_mi355x.h")
    for name in NAMES:
        assert name in scn.EXPORTS
        assert re.search(r"^int " + name + r"\(const uint16_t\* X, ", header, re.M), name
    # the fp32 twins' argument lists: (X, count, Y, stream) and (X, dY, count, dX, stream)
    assert L._SIGS["scn_relu_fwd_bf16"] == L._SIGS["scn_relu_fwd"]
    assert L._SIGS["scn_relu_bwd_bf16"] == L._SIGS["scn_relu_bwd"]


def test_documents_quote_the_entry_point_count():
    import sparse_rcnn_amd as scn
    n = len(scn.EXPORTS)
    header = _read("include", "scn_mi355x.h")
    history = header[:header.index("#define SCN_ABI_VERSION")]
    assert int(re.findall(r"\((\d+) entry\s+\*?\s*points\)", history)[-1]) == n            # the last line of the ABI history
    assert NAMES[0] in history
    assert f"`include/scn_mi355x.h`, {n} entry points" in _read("README.md")
    assert f"`include/scn_mi355x.h` ({n} `extern \"C\"` entry points" in _read("DESIGN.md")
    assert f"{n} entry points" in _read("INTEGRATION.md")


def test_multilevel_rpn_takes_the_upsampling_heads_with_a_bf16_stack():
    from sparse_rcnn_amd import rpn as R
    up_levels = [(8, 4, 8, R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS[0]), (8, 8, 8, R.REF_UPSAMPLE_ANCHOR_LEVELS_VOXELS[1])]
    torch.manual_seed(3)
    up = R.MultiLevelRpn(up_levels, num_dilations=1, autocast_bf16=True, extra_stride_levels=R.REF_EXTRA_STRIDE_LEVELS)
    names = [k for k, _ in up.named_parameters()]
    assert not any(".head." in k for k in names) and all(l.head is None and l.autocast_bf16 for l in up.levels)
    assert up.anchor_network is not None
    # the same modules and seeded values as without the switch: it chooses a storage arrangement, not a network
    torch.manual_seed(3)
    f32 = R.MultiLevelRpn(up_levels, num_dilations=1, extra_stride_levels=R.REF_EXTRA_STRIDE_LEVELS)
    assert names == [k for k, _ in f32.named_parameters()]
    assert all(torch.equal(a, b) for a, b in zip(up.parameters(), f32.parameters()))
