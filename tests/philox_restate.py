"""An independent restatement of the sample conversion's generator and of the random cut-out on it: Python integers and
float64 only, nothing imported from the package.

Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): per round
(c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key moves by the Weyl constants
between rounds.  The project maps key = (seed lo32, seed hi32), counter = (index, stream, sample counter lo32, hi32)."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
    return (c0, c1, c2, c3)


def words(seed, counter, stream, index):
    return philox4x32_10((index & MASK, stream & MASK, counter & MASK, (counter >> 32) & MASK), (seed & MASK, (seed >> 32) & MASK))


def uniform(w):
    return ((w >> 9) + 0.5) * 2.0 ** -23


def normals(w):
    """The three normals of one draw in float64."""
    r0, r1 = math.sqrt(-2 * math.log(uniform(w[0]))), math.sqrt(-2 * math.log(uniform(w[2])))
    return (r0 * math.cos(2 * math.pi * uniform(w[1])), r0 * math.sin(2 * math.pi * uniform(w[1])),
            r1 * math.cos(2 * math.pi * uniform(w[3])))


def words_array(seed, counter, stream, first, n):
    """uint32 [n][4] of indices first .. first + n - 1: the same rounds on numpy uint64 columns (every product of two 32-bit
    values fits), checked against `words` by the tests."""
    c = [np.arange(first, first + n, dtype=np.uint64) & np.uint64(MASK), np.full(n, stream, np.uint64),
         np.full(n, counter & MASK, np.uint64), np.full(n, counter >> 32, np.uint64)]
    k0, k1 = seed & MASK, seed >> 32
    sh, mk = np.uint64(32), np.uint64(MASK)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & mk, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & mk]
    return np.stack(c, 1).astype(np.uint32)


def normals_array(w):
    """float64 [n][3] from uint32 [n][4]."""
    u = ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r0, r1 = np.sqrt(-2 * np.log(u[:, 0])), np.sqrt(-2 * np.log(u[:, 2]))
    return np.stack([r0 * np.cos(2 * np.pi * u[:, 1]), r0 * np.sin(2 * np.pi * u[:, 1]), r1 * np.cos(2 * np.pi * u[:, 3])], 1)


CUT_STREAM = 1


def random_cut_out(discrete, size, border, seed, counter):
    """random_cut_out (ndsis/data/sparse_augmentation.py:50-78) with its line 76 applied to a clone, in numpy, its three draws
    replaced by words: the order from (stream 1, index 0) -- i = (w0 * 3) >> 32, j = (w1 * 2) >> 32 popped from [0, 1, 2] -- and
    the start of the k-th dimension of that order from word k of (stream 1, index 1), min_start + ((w * span) >> 32).
    -> (start [3], order [3], voxels alive after the last processed dimension, dimensions processed, is_inside bool [N])."""
    discrete = np.asarray(discrete, dtype=np.int64)
    w_order, w_start = words(seed, counter, CUT_STREAM, 0), words(seed, counter, CUT_STREAM, 1)
    rest = [0, 1, 2]
    order = [rest.pop((w_order[0] * 3) >> 32), rest.pop((w_order[1] * 2) >> 32), rest[0]]
    start = [0, 0, 0]
    is_inside = np.ones(discrete.shape[0], dtype=bool)
    inside = discrete.copy()
    processed = 0
    for k, dim in enumerate(order):
        if not len(inside):
            break
        lo = int(inside[:, dim].min()) - border[dim]
        hi = int(inside[:, dim].max()) + 1 - size[dim] + border[dim]
        if hi <= lo:
            start[dim] = lo
            inside[:, dim] -= start[dim]
        else:
            start[dim] = lo + ((w_start[k] * (hi - lo)) >> 32)
            inside[:, dim] -= start[dim]
            remaining = (0 <= inside[:, dim]) & (inside[:, dim] < size[dim])
            inside = inside[remaining]
            is_inside[is_inside.copy()] = remaining
        processed = k + 1
    return start, order, len(inside), processed, is_inside
