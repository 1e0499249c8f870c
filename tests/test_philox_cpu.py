"""The sample conversion's counter-based generator, host side (no GPU): Random123's known-answer vectors for Philox4x32-10
against the independent restatement (tests/philox_restate.py), the package's numpy form (sample.philox_words) and the C header
compiled for the host (scn_philox_words_host); the moments of the normals; the restated random cut-out on words against the
restatement the host-generator path is pinned to; PhiloxDraws' host values; the new entry points' status codes."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import philox_restate as P                                     # noqa: E402
import sample_restate as R                                     # noqa: E402

# Random123 (kat_vectors, philox4x32 10): counter; key -> words
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
SPECIFIC = ((1234, 7, 2, 0), (0x3974ec34, 0x9db2f39d, 0x06b25535, 0x5974d679))


def _project_args(counter, key):
    """(counter; key) as the project's (seed, sample counter, stream, index)."""
    return key[0] | (key[1] << 32), counter[2] | (counter[3] << 32), counter[1], counter[0]


def _c_words(seed, counter, stream, index):
    from sparse_rcnn_amd import _lib as L
    out = (C.c_uint32 * 4)()
    assert L.load().scn_philox_words_host(seed, counter, stream, index, out) == L.OK
    return tuple(out)


@pytest.mark.parametrize("counter,key,want", KAT)
def test_known_answer_vectors(counter, key, want):
    from sparse_rcnn_amd.sample import philox_words
    assert P.philox4x32_10(counter, key) == want
    args = _project_args(counter, key)
    assert P.words(*args) == want
    got = philox_words(*args)
    assert got.dtype == np.uint32 and got.shape == (4,) and tuple(int(v) for v in got) == want
    assert _c_words(*args) == want


def test_specific_words_and_array_forms():
    from sparse_rcnn_amd.sample import philox_words
    args, want = SPECIFIC
    assert P.words(*args) == want and _c_words(*args) == want
    assert tuple(int(v) for v in philox_words(*args)) == want
    for seed, counter, stream in ((1234, 7, 2), (2 ** 63 + 5, 2 ** 40 + 1, 3), (2 ** 64 - 1, 2 ** 64 - 1, 5)):
        arr = P.words_array(seed, counter, stream, 5, 70)
        pkg = philox_words(seed, counter, stream, np.arange(5, 75))
        assert pkg.shape == (70, 4) and np.array_equal(arr, pkg)
        for i in (0, 1, 63, 69):
            assert tuple(int(v) for v in arr[i]) == P.words(seed, counter, stream, 5 + i) == _c_words(seed, counter, stream, 5 + i)
    # index and stream broadcast against each other
    both = philox_words(9, 3, np.arange(6)[:, None], np.arange(4)[None, :])
    assert both.shape == (6, 4, 4) and tuple(int(v) for v in both[5, 2]) == P.words(9, 3, 5, 2)


def test_uniform_and_normals_of_the_package_equal_the_restatement():
    from sparse_rcnn_amd.sample import philox_normals
    assert P.uniform(0) == 2.0 ** -24 and P.uniform(0xFFFFFFFF) == 1 - 2.0 ** -24          # inside (0, 1), never 0
    assert float(np.float32(P.uniform(0xFFFFFFFF))) == P.uniform(0xFFFFFFFF)                 # exact in fp32
    z = philox_normals(1234, 7, 2, np.arange(50))
    assert z.dtype == np.float32 and z.shape == (50, 3)
    ref = np.array([P.normals(P.words(1234, 7, 2, i)) for i in range(50)])
    assert np.array_equal(z, ref.astype(np.float32))
    assert np.array_equal(P.normals_array(P.words_array(1234, 7, 2, 0, 50)), ref)


@pytest.mark.parametrize("seed,counter,stream", [(1234, 7, 2), (0, 0, 3), (2 ** 63 + 5, 2 ** 40 + 1, 2)])
def test_moments_of_the_normals(seed, counter, stream):
    rows = 1 << 18
    z = P.normals_array(P.words_array(seed, counter, stream, 0, rows))
    n = z.size
    mean, var = float(z.mean()), float(z.var())
    corr = np.corrcoef(z.T)
    worst = float(np.abs(corr[np.triu_indices(3, 1)]).max())
    print(f"[moments] ({seed}, {counter}, {stream}): |mean| {abs(mean):.4f}  |var - 1| {abs(var - 1):.4f}  correlation {worst:.4f}")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert worst <= 5 / math.sqrt(rows)


def test_restated_cut_out_by_hand():
    """Four voxels on a line in x, size (2, 9, 9), no border: x has the range [0, 5), y and z have extent 1 < 9, an empty
    range, so their start is min_start = 0 and they cut nothing.  The restatement's answer, followed step by step."""
    pts = np.array([[0, 0, 0], [1, 0, 0], [5, 0, 0], [6, 0, 0]])
    for seed, counter in ((3, 0), (3, 1), (2 ** 64 - 1, 2 ** 50)):
        start, order, alive, dims, inside = P.random_cut_out(pts, [2, 9, 9], [0, 0, 0], seed, counter)
        w0, w1 = P.words(seed, counter, 1, 0), P.words(seed, counter, 1, 1)
        rest = [0, 1, 2]
        want_order = [rest.pop((w0[0] * 3) >> 32), rest.pop((w0[1] * 2) >> 32)] + rest
        assert order == want_order and sorted(order) == [0, 1, 2]
        x0 = (w1[order.index(0)] * 5) >> 32                     # the word of x's POSITION in the order
        assert start == [x0, -8 + 8, -8 + 8] and 0 <= x0 < 5
        want_inside = (pts[:, 0] - x0 >= 0) & (pts[:, 0] - x0 < 2)
        assert np.array_equal(inside, want_inside) and alive == int(want_inside.sum())
        # a window in the gap (x0 = 2 or 3) leaves nothing alive: the loop stops after x, later dimensions are not processed
        assert dims == (3 if alive else order.index(0) + 1)


class _Order:
    """What the patched torch.multinomial returns: iterates like the tensor of dimensions and tells the patched randint
    which position of the order the loop is at."""

    def __init__(self, order, state):
        self.order, self.state = order, state

    def __iter__(self):
        for k, d in enumerate(self.order):
            self.state["k"] = k
            yield torch.tensor(d)


@pytest.mark.parametrize("case", range(12))
def test_restated_cut_out_equals_the_torch_restatement_fed_the_same_draws(case, monkeypatch):
    """tests/sample_restate.py random_cut_out -- what the host-generator path is pinned to -- with torch.multinomial and
    torch.randint replaced by the order and the starts the words give, against the numpy restatement on words."""
    rng = np.random.default_rng(case)
    n = int(rng.integers(1, 3000))
    size = [int(v) for v in rng.integers(4, 40, size=3)]
    extent = [max(1, s + int(rng.integers(-3, 90))) for s in size]         # some axes shorter than the size: no draw there
    pts = rng.integers(0, extent, size=(n, 3)).astype(np.int64)
    border = [0, 0, 0] if case % 2 else [s // 4 for s in size]
    seed, counter = 77 + case, 2 ** 33 + case
    start, order, alive, dims, inside = P.random_cut_out(pts, size, border, seed, counter)
    w1 = P.words(seed, counter, 1, 1)
    state = {}

    def fake_randint(lo, hi, shape):
        assert hi > lo and shape == ()
        return torch.tensor(lo + ((w1[state["k"]] * (hi - lo)) >> 32))

    monkeypatch.setattr(torch, "multinomial", lambda w, k: _Order(order, state))
    monkeypatch.setattr(torch, "randint", fake_randint)
    start_ref, inside_ref, coords_ref = R.random_cut_out(torch.from_numpy(pts), torch.tensor(size), border)
    monkeypatch.undo()
    assert start_ref.tolist() == start
    assert np.array_equal(inside_ref.numpy(), inside) and alive == int(inside.sum()) == coords_ref.shape[0]
    assert dims == 3 if alive else 1 <= dims <= 3


def test_philox_draws_host_part():
    from sparse_rcnn_amd.sample import Draws, PhiloxDraws, philox_normals, philox_words
    a, b, c = PhiloxDraws(11, 5, coord_noise_sigma=0.1), PhiloxDraws(11, 5, coord_noise_sigma=0.1), PhiloxDraws(11, 6, coord_noise_sigma=0.1)
    assert isinstance(a, Draws) and a.almost_orthonormal.dtype == torch.float32 and a.almost_orthonormal.shape == (3, 3)
    assert torch.equal(a.almost_orthonormal, b.almost_orthonormal) and torch.equal(a.sub_pixel_offset, b.sub_pixel_offset)
    assert not torch.equal(a.almost_orthonormal, c.almost_orthonormal) and not torch.equal(a.sub_pixel_offset, c.sub_pixel_offset)
    assert a.start_positions is None and a.color_noise is None and a.normal_noise is None
    assert bool(((a.sub_pixel_offset > 0) & (a.sub_pixel_offset < 1)).all())
    # the stated recipe: normals of indices 0 .. 2, mirror bit and angle of index 3, offset of index 4, all of stream 0
    z = torch.from_numpy(philox_normals(11, 5, 0, np.arange(3)))
    w = philox_words(11, 5, 0, np.arange(3, 5))
    m = torch.eye(3) + z * 0.1
    m[0, 0] *= int(w[0, 0] & 1) * 2 - 1
    angle = torch.tensor(P.uniform(int(w[0, 1])), dtype=torch.float32) * 2 * math.pi
    cs, sn = torch.cos(angle), torch.sin(angle)
    assert torch.equal(a.almost_orthonormal, m @ torch.tensor([[cs, sn, 0.], [-sn, cs, 0.], [0., 0., 1.]]))
    assert a.sub_pixel_offset.tolist() == [float(np.float32(P.uniform(int(v)))) for v in w[1, :3]]
    # fixed values pass through; nothing random is left with sigma 0
    fixed = PhiloxDraws(11, 5, coord_noise_sigma=0, theta=0.0, mirror=False, sub_pixel_offset=torch.tensor([0.25, 0.5, 0.75]))
    assert torch.equal(fixed.almost_orthonormal, torch.eye(3)) and fixed.sub_pixel_offset.tolist() == [0.25, 0.5, 0.75]
    mirrored = PhiloxDraws(11, 5, coord_noise_sigma=0, theta=0.0, mirror=True)
    assert torch.equal(mirrored.almost_orthonormal, torch.diag(torch.tensor([-1., 1., 1.])))
    quarter = PhiloxDraws(11, 5, coord_noise_sigma=0, theta=math.pi / 2, mirror=False)
    want = torch.tensor([[math.cos(math.pi / 2), 1., 0.], [-1., math.cos(math.pi / 2), 0.], [0., 0., 1.]])
    assert torch.allclose(quarter.almost_orthonormal, want, atol=1e-7)
    # a list of angles: the pick is (w * len) >> 32 of word 1 of index 3; both mirror values occur over counters
    angles = [0.0, 1.0, 2.0, 3.0]
    picks = set()
    for counter in range(40):
        d = PhiloxDraws(5, counter, theta=angles, mirror=False)
        k = (int(philox_words(5, counter, 0, 3)[1]) * 4) >> 32
        picks.add(k)
        assert abs(float(d.almost_orthonormal[0, 0]) - math.cos(angles[k])) < 1e-6
    assert picks == {0, 1, 2, 3}
    assert {float(PhiloxDraws(5, k, theta=0.0).almost_orthonormal[0, 0]) for k in range(40)} == {-1.0, 1.0}


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    from sparse_rcnn_amd import _lib as L
    lib = L.load()
    buf = (C.c_int32 * 64)()
    p = C.addressof(buf)
    assert lib.scn_philox_words_host(1, 2, 3, 4, None) == L.EINVAL
    assert lib.scn_philox_fill(1, 2, 2, 0, -1, 0, 1.0, p, None) == L.EINVAL                          # n < 0
    assert lib.scn_philox_fill(1, 2, 2, -1, 4, 0, 1.0, p, None) == L.EINVAL
    assert lib.scn_philox_fill(1, 2, 2, 0, 4, 2, 1.0, p, None) == L.EINVAL                           # no such mode
    assert lib.scn_philox_fill(1, 2, 2, 0, 4, 1, 1.0, None, None) == L.EINVAL
    assert lib.scn_philox_fill(1, 2, 2, 2 ** 32 - 3, 4, 0, 1.0, p, None) == L.ESIZE                  # index word overflows
    assert b"32-bit index" in lib.scn_last_error_string()
    assert lib.scn_philox_fill(1, 2, 2, 5, 0, 1, 1.0, None, None) == L.OK                            # n = 0: nothing to do
    rot = (C.c_float * 9)()
    tail = (1, 1, 1, p, p, p, p, 1, p, None)
    drawn = (7, 9, 0.1, 0, 0.0, 0)
    assert lib.scn_sample_pack_drawn(p, -1, p, p, p, 3, rot, *drawn, *tail) == L.EINVAL
    assert lib.scn_sample_pack_drawn(p, 0, p, p, p, 3, rot, *drawn, *tail) == L.OK                   # M = 0: nothing to do
    assert lib.scn_sample_pack_drawn(p, 8, p, p, p, L.SAMPLE_MAX_INSTANCES + 1, rot, *drawn, *tail) == L.ESIZE
    assert b"scn_sample_pack_drawn" in lib.scn_last_error_string()
    assert lib.scn_sample_pack_drawn(p, 8, p, p, p, 3, rot, *drawn, 1, 1, 1, None, p, p, p, 1, p, None) == L.EINVAL
    assert lib.scn_sample_pack_drawn(p, 8, p, p, p, 3, rot, 7, 9, float("nan"), 0, 0.0, 0, *tail) == L.EINVAL
    size, border, zero = (C.c_int32 * 3)(32, 32, 16), (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(32, 0, 16)
    assert lib.scn_sample_cut_start(p, 0, size, border, 1, 2, p, None) == L.EINVAL                   # N = 0
    assert lib.scn_sample_cut_start(p, 8, zero, border, 1, 2, p, None) == L.EINVAL                   # a size < 1
    assert lib.scn_sample_cut_start(p, 8, size, (C.c_int32 * 3)(0, 33, 0), 1, 2, p, None) == L.EINVAL   # a border above the size
    assert lib.scn_sample_cut_start(p, 8, size, (C.c_int32 * 3)(0, -1, 0), 1, 2, p, None) == L.EINVAL
    assert lib.scn_sample_cut_start(None, 8, size, border, 1, 2, p, None) == L.EINVAL
    assert lib.scn_sample_cut_start(p, 8, size, border, 1, 2, None, None) == L.EINVAL
