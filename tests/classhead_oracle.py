"""The class branch and the segmentation head restated on the oracle's operators (oracle/scn_oracle.py as it stands: conv,
subm_rulebook, strided_rulebook, transform_boxes with clip and resize, roi_crop, input_layer_rules, global_pool,
output_layer_fwd) -- the checker of tests/test_gpu_class_loss.py."""
import numpy as np
import torch

from oracle import scn_oracle as O


def _residual(x, P, prefix, rules, n, relu):
    y = O.conv(relu(x), P[f"{prefix}.conv0.weight"], P[f"{prefix}.conv0.bias"], rules, n)
    y = O.conv(relu(y), P[f"{prefix}.conv1.weight"], P[f"{prefix}.conv1.bias"], rules, n)
    return x + y


def class_branch(coords, X, P, boxes, spatial_size, stride, relu=None, n_levels=2):
    """coords int64 [N, 4]: the active sites of the feature map in row order; X [N, C]; P: ClassBranch.named_oracle_params
    on the host; boxes: list (one per sample) of fp32 [n, 2, 3] in scene units.
    -> (scores [BB, classes], src_row, box_of, rows per box)."""
    relu = torch.relu if relu is None else relu
    coords = np.asarray(coords, dtype=np.int64)
    n = len(coords)
    ident = [(np.arange(n, dtype=np.int32),) * 2]
    x = O.conv(X, P["in.weight"], P["in.bias"], ident, n)
    x = _residual(x, P, "in.res0", O.subm_rulebook(coords, 3)[1], n, relu)
    boxes_int, counts, assoc = O.transform_boxes([np.asarray(b) for b in boxes], spatial_size, clip=True, resize=stride)
    src, box_of, inside = O.roi_crop(coords, boxes_int, assoc)
    roi_coords = np.concatenate([coords[src, :3], box_of[:, None]], 1)
    level, prow, _ = O.input_layer_rules(roi_coords)            # mode 0: the sites of a box are unique
    assert len(level) == len(roi_coords) and np.array_equal(prow, np.arange(len(prow)))
    x = x[torch.from_numpy(src)]
    for l in range(n_levels):
        rb = O.strided_rulebook(level, 2)
        level = rb["coords"]
        x = O.conv(x, P[f"down{l}.weight"], P[f"down{l}.bias"], rb["rules"], len(level))
        x = _residual(x, P, f"down{l}.res0", O.subm_rulebook(level, 3)[1], len(level), relu)
    pooled = O.global_pool(x, level, len(boxes_int), torch.mean)
    h = relu(pooled) @ P["lin0.weight"].t() + P["lin0.bias"]
    scores = relu(h) @ P["lin1.weight"].t() + P["lin1.bias"]
    return scores, src, box_of, inside.sum(1)


def segmentation_head(X, prow, W, b):
    n = X.shape[0]
    ident = [(np.arange(n, dtype=np.int32),) * 2]
    return O.output_layer_fwd(O.conv(X, W, b, ident, n), prow)
