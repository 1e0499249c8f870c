"""float64 numpy restatement of the executor's two gradient-clipping ops (include/scn_mi355x.h: SCN_OP_GRAD_NORM,
SCN_OP_GRAD_SCALE) and of the fp32 arithmetic of the clip coefficient.  Not a test itself: tests/test_clip_cpu.py checks it
against torch.nn.utils.clip_grad_norm_ on float64 CPU tensors, tests/test_gpu_clip.py checks the kernels against it."""
import numpy as np


def sum_squares(segments):
    """Sum of squares of every element of every segment, in float64."""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(sum(np.sum(np.square(np.asarray(s, dtype=np.float64).reshape(-1))) for s in segments))


def total_norm(segments, grad_scale=1.0):
    """sqrt(sum of squares) x |grad_scale| in float64: what SCN_OP_GRAD_NORM rounds to fp32 once."""
    with np.errstate(invalid="ignore"):
        return float(np.sqrt(np.float64(sum_squares(segments))) * abs(np.float64(np.float32(grad_scale))))


def coef_f32(total, max_norm):
    """The clip coefficient from an fp32 total norm, in fp32 as torch computes it on fp32 gradients:
    c = max_norm / (total + 1e-6), then min(c, 1) where a NaN stays a NaN (torch.clamp)."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = np.float32(max_norm) / (np.float32(total) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else np.float32(c)


def record(segments, max_norm, grad_scale=1.0):
    """(total_norm as fp32, clip_coef as fp32, nonfinite) -- the record SCN_OP_GRAD_NORM writes."""
    with np.errstate(over="ignore", invalid="ignore"):
        total = np.float32(total_norm(segments, grad_scale))
    return total, coef_f32(total, max_norm), float(not np.isfinite(sum_squares(segments)))


def scaled_f32(segment, coef):
    """SCN_OP_GRAD_SCALE on one fp32 segment: one fp32 multiply per element."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(segment, dtype=np.float32) * np.float32(coef)


def clip_f64(segments, max_norm):
    """torch.nn.utils.clip_grad_norm_ restated entirely in float64 (for float64 gradients): -> (total norm, scaled segments)."""
    total = total_norm(segments)
    with np.errstate(invalid="ignore"):
        c = np.float64(max_norm) / (np.float64(total) + np.float64(1e-6))
        c = np.float64(1.0) if c > 1.0 else c
        return total, [np.asarray(s, dtype=np.float64) * c for s in segments]
