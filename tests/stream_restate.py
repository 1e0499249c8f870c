"""Plain numpy / float64 restatement of the streaming and row-movement operations (csrc/scn_elem.hip, scn_elem_bf16.hip,
scn_segpool.hip, the column sum of scn_conv.hip), written from the kernels' stated contracts, not from their code.
TEST INFRASTRUCTURE ONLY: tests/test_stream_restate_cpu.py pins it against the oracle and torch, tests/test_gpu_streaming.py
holds the kernels to it.

Values go in and come out as numpy arrays.  Every function computes in float64 and leaves rounding to the caller, except
where the contract itself fixes a rounding (`segment_sum`: the float64 sum rounded ONCE to fp32, for bf16 then to bf16).
"""
from __future__ import annotations

import numpy as np


# ---- bf16 <-> fp32 on bit patterns (round-to-nearest-even; NaN stays NaN) -------------------------------------------
def bf16_bits_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(x):
    """Round-to-nearest-even of fp32 to bf16 bit patterns; NaN -> a quiet NaN of the same sign."""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r[nan] = ((u[nan] >> 16) | 0x0040).astype(np.uint16)
    return r


def round_bf16(x):
    """fp32-representable values of x after one bf16 rounding (as float64)."""
    return bf16_bits_to_f32(f32_to_bf16_bits(np.asarray(x, dtype=np.float32))).astype(np.float64)


# ---- MaxPooling / AveragePooling on the child table [n_off, n_coarse] (-1: no child) -------------------------------
def pool_fwd(X, child, average):
    """max: Y = max(0, max over existing children);  avg: Y = (sum over existing children) / n_off.  float64 [n_coarse, c]."""
    X = np.asarray(X, dtype=np.float64)
    n_off, nc = child.shape
    Y = np.zeros((nc, X.shape[1]), dtype=np.float64)
    for o in range(n_off):
        rows = np.nonzero(child[o] >= 0)[0]
        v = X[child[o][rows]]
        if average:
            Y[rows] += v
        else:
            Y[rows] = np.where(v > Y[rows], v, Y[rows])          # the output starts at +0 and only a greater value replaces it
    return Y / float(n_off) if average else Y


def pool_bwd(X, Y, dY, parent, average, n_off):
    """max: dX[f] = dY[parent[f]] where X[f] == Y[parent[f]] AS VALUES (every tied child gets the full dY; -0 == +0), else 0;
    avg: dX[f] = dY[parent[f]] / n_off."""
    dY = np.asarray(dY, dtype=np.float64)
    g = dY[np.asarray(parent, dtype=np.int64)]
    if average:
        return g / float(n_off)
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    return np.where(X == Y[np.asarray(parent, dtype=np.int64)], g, 0.0)


def pool_tie_cells(X, child):
    """bool [n_coarse, c]: the cell's maximum max(0, children) is attained by MORE than one child."""
    Y = pool_fwd(X, child, False)
    X = np.asarray(X, dtype=np.float64)
    hits = np.zeros(Y.shape, dtype=np.int64)
    for o in range(child.shape[0]):
        rows = np.nonzero(child[o] >= 0)[0]
        hits[rows] += X[child[o][rows]] == Y[rows]
    return hits > 1


# ---- SparseToDense: out[b][ch][x][y][z] --------------------------------------------------------------------------------
def sparse_to_dense_fwd(X, coords, size, batch):
    """Index put into zeros [batch, c, sx, sy, sz]; coords [n, 4] = (x, y, z, sample)."""
    X = np.asarray(X)
    c = np.asarray(coords, dtype=np.int64)
    out = np.zeros((batch, X.shape[1]) + tuple(int(s) for s in size), dtype=X.dtype)
    out[c[:, 3], :, c[:, 0], c[:, 1], c[:, 2]] = X
    return out


def sparse_to_dense_bwd(dOut, coords):
    """Index get: dX[r] = dOut[sample, :, x, y, z]."""
    c = np.asarray(coords, dtype=np.int64)
    return np.asarray(dOut)[c[:, 3], :, c[:, 0], c[:, 1], c[:, 2]]


# ---- row gather / segment sum ------------------------------------------------------------------------------------------
def gather_rows(X, rows):
    return np.asarray(X)[np.asarray(rows, dtype=np.int64)]


def segment_sum(V, item_row, n_rows, bf16=False):
    """out[row] = sum of V[item] over the items of that row: the float64 sum rounded ONCE to fp32 (fp32 array), and for
    bf16 storage (V = bit patterns) that fp32 value rounded to bf16 (bit patterns)."""
    v = bf16_bits_to_f32(V).astype(np.float64) if bf16 else np.asarray(V, dtype=np.float64)
    acc = np.zeros((int(n_rows), v.shape[1]), dtype=np.float64)
    np.add.at(acc, np.asarray(item_row, dtype=np.int64), v)
    out = acc.astype(np.float32)
    return f32_to_bf16_bits(out) if bf16 else out


# ---- column sum --------------------------------------------------------------------------------------------------------
def colsum(dY):
    """(sum over rows, sum over rows of |.|) in float64."""
    d = np.asarray(dY, dtype=np.float64)
    return d.sum(0), np.abs(d).sum(0)


# ---- per-sample mean / sum / amax --------------------------------------------------------------------------------------
def _total_order_key(x):
    """float64 -> int64 key of the IEEE total order restricted to non-NaN values: -0 sorts below +0."""
    i = np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)
    return np.where(i >= 0, i, i ^ np.int64(0x7FFFFFFFFFFFFFFF))


def segment_pool_fwd(X, sample, n_samples, op):
    """op in ("mean", "sum", "amax").  float64 [n_samples, c]; a sample without rows pools to zeros.  amax is the true maximum
    (negative for an all-negative sample); among a -0 / +0 pair it is +0."""
    X = np.asarray(X, dtype=np.float64)
    sample = np.asarray(sample, dtype=np.int64)
    Y = np.zeros((n_samples, X.shape[1]), dtype=np.float64)
    for b in range(n_samples):
        x = X[sample == b]
        if not len(x):
            continue
        if op == "amax":
            Y[b] = np.take_along_axis(x, _total_order_key(x).argmax(0)[None], 0)[0]
        else:
            Y[b] = x.sum(0) / (len(x) if op == "mean" else 1)
    return Y


def segment_pool_bwd(X, Y, dY, sample, n_samples, op):
    """fp32 [n, c], rounded as the contract states: mean dY / float(cnt), sum a copy of dY, amax dY / ties for the rows that
    equal the maximum AS VALUES (evenly among equal maxima), 0 elsewhere."""
    X, Y = np.asarray(X, dtype=np.float32), np.asarray(Y, dtype=np.float32)
    dY = np.asarray(dY, dtype=np.float32)
    sample = np.asarray(sample, dtype=np.int64)
    dX = np.zeros(X.shape, dtype=np.float32)
    for b in range(n_samples):
        m = sample == b
        cnt = int(m.sum())
        if not cnt:
            continue
        if op == "mean":
            dX[m] = (dY[b] / np.float32(cnt))[None]
        elif op == "sum":
            dX[m] = dY[b][None]
        else:
            hit = X[m] == Y[b][None]
            ties = hit.sum(0)
            dX[m] = np.where(hit, (dY[b] / np.maximum(ties, 1).astype(np.float32))[None], np.float32(0))
    return dX
