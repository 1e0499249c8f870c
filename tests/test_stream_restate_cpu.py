"""Pins tests/stream_restate.py (the numpy / float64 restatement the GPU streaming tests compare against) on the CPU:
against the oracle, against torch's dense twins, and -- for the max-pool gradient -- against autograd of `O.pool_fwd`, with
the one place where the upstream rule and autograd part ways (a tie) recorded explicitly."""
import numpy as np
import pytest
import torch

import stream_restate as R
from oracle import scn_oracle as O


def _scene(seed, grid=(12, 12, 12), n=300, batch=2):
    rng = np.random.default_rng(seed)
    cs = []
    for b in range(batch):
        lin = rng.choice(grid[0] * grid[1] * grid[2], size=n, replace=False)
        p = np.stack(np.unravel_index(lin, grid), 1)
        cs.append(np.concatenate([p, np.full((n, 1), b)], 1))
    return np.concatenate(cs).astype(np.int64), grid, batch


STRIDES = [(2, 2, 2), (3, 3, 3), (2, 2, 1), (1, 2, 3), (4, 4, 4)]


@pytest.mark.parametrize("stride", STRIDES)
def test_pool_forward_equals_the_oracle_and_the_dense_twin(stride):
    coords, grid, batch = _scene(1)
    rb = O.strided_rulebook(coords, stride)
    X = torch.randn(len(coords), 5, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    for average in (False, True):
        y = R.pool_fwd(X.numpy(), rb["child"], average)
        yo = O.pool_fwd(X, rb["child"], average).numpy()
        if average:
            np.testing.assert_allclose(y, yo, rtol=0, atol=1e-14)         # (the oracle divides every term, the restatement the sum)
        else:
            assert np.array_equal(y, yo)
    # average pooling == avg_pool3d of the zero-filled grid, sampled at the coarse sites
    dense = torch.from_numpy(R.sparse_to_dense_fwd(X.numpy(), coords, grid, batch))
    dd = torch.nn.functional.avg_pool3d(dense, stride, stride).numpy()
    c = rb["coords"]
    np.testing.assert_allclose(R.pool_fwd(X.numpy(), rb["child"], True), dd[c[:, 3], :, c[:, 0], c[:, 1], c[:, 2]],
                               rtol=0, atol=1e-14)


@pytest.mark.parametrize("stride", STRIDES)
def test_pool_backward_equals_autograd_of_the_oracle_without_ties(stride):
    coords, grid, batch = _scene(3)
    rb = O.strided_rulebook(coords, stride)
    n_off = rb["child"].shape[0]
    X = torch.randn(len(coords), 5, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    assert not R.pool_tie_cells(X.numpy(), rb["child"]).any()
    for average in (False, True):
        Xo = X.clone().requires_grad_()
        yo = O.pool_fwd(Xo, rb["child"], average)
        g = torch.randn(yo.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
        (ag,) = torch.autograd.grad(yo, Xo, g)
        dx = R.pool_bwd(X.numpy(), yo.detach().numpy(), g.numpy(), rb["parent"], average, n_off)
        np.testing.assert_allclose(dx, ag.numpy(), rtol=0, atol=1e-15 if average else 0)
        ob = O.pool_bwd(X, yo.detach(), g, rb["parent"], average, n_off)
        assert np.array_equal(ob.numpy(), dx)


def test_max_pool_backward_gives_full_dy_to_every_tied_child_where_autograd_splits_it():
    """One 2^3 cell with four children, channel 0: two children tie at the maximum 1.5; channel 1: every child is 0 (the
    cell's output is the initial zero); channel 2: a -0 and a +0 child below nothing else; channel 3: no tie."""
    coords = np.array([[0, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [1, 1, 1, 0]], dtype=np.int64)
    rb = O.strided_rulebook(coords, 2)
    assert rb["child"].shape == (8, 1)
    X = torch.tensor([[1.5, 0.0, -0.0, 1.0],
                      [1.5, 0.0, 0.0, 2.0],
                      [0.5, 0.0, -1.0, 3.0],
                      [-1.0, 0.0, -2.0, -4.0]], dtype=torch.float64)
    g = torch.tensor([[2.0, 3.0, 5.0, 7.0]], dtype=torch.float64)
    Y = R.pool_fwd(X.numpy(), rb["child"], False)
    assert np.array_equal(Y, [[1.5, 0.0, 0.0, 3.0]]) and not np.signbit(Y).any()
    assert R.pool_tie_cells(X.numpy(), rb["child"]).tolist() == [[True, True, True, False]]
    dx = R.pool_bwd(X.numpy(), Y, g.numpy(), rb["parent"], False, 8)
    want = np.array([[2.0, 3.0, 5.0, 0.0],
                     [2.0, 3.0, 5.0, 0.0],
                     [0.0, 3.0, 0.0, 7.0],
                     [0.0, 3.0, 0.0, 0.0]])
    assert np.array_equal(dx, want)
    assert np.array_equal(O.pool_bwd(X, torch.from_numpy(Y), g, rb["parent"], False, 8).numpy(), want)
    # autograd of O.pool_fwd: the same support on the untied channel, but a tie is NOT handed the full dY by every path
    Xo = X.clone().requires_grad_()
    (ag,) = torch.autograd.grad(O.pool_fwd(Xo, rb["child"], False), Xo, g)
    ag = ag.numpy()
    assert np.array_equal(ag[:, 3], want[:, 3])
    for ch in (0, 1, 2):
        assert ag[:, ch].sum() <= g[0, ch].item() + 1e-12 < want[:, ch].sum()       # autograd conserves dY; upstream multiplies it
        assert not np.array_equal(ag[:, ch], want[:, ch])


def test_bf16_rounding_and_segment_sum_match_torch():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(4000, generator=g) * 3, torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 1e-40, 3.4e38,
                                                                     1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])])
    bits = R.f32_to_bf16_bits(x.numpy())
    assert np.array_equal(bits, x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(R.bf16_bits_to_f32(bits), x.to(torch.bfloat16).float().numpy())
    assert np.isnan(R.bf16_bits_to_f32(R.f32_to_bf16_bits(np.array([np.nan], dtype=np.float32)))).all()
    rows = torch.randint(0, 50, (700,), generator=g)
    v = torch.randn(700, 3, generator=g)
    exp = torch.zeros(50, 3, dtype=torch.float64).index_add_(0, rows, v.double())
    assert np.array_equal(R.segment_sum(v.numpy(), rows.numpy(), 50), exp.float().numpy())
    vb = v.to(torch.bfloat16)
    expb = torch.zeros(50, 3, dtype=torch.float64).index_add_(0, rows, vb.double()).float().to(torch.bfloat16)
    assert np.array_equal(R.segment_sum(vb.view(torch.int16).numpy().view(np.uint16), rows.numpy(), 50, bf16=True),
                          expb.view(torch.int16).numpy().view(np.uint16))


def test_sparse_to_dense_and_global_pool_match_the_oracle():
    coords, grid, batch = _scene(7, grid=(5, 7, 3), n=40, batch=3)
    coords = coords[coords[:, 3] != 1]                                     # the middle sample is empty
    X = torch.randn(len(coords), 6, generator=torch.Generator().manual_seed(8))
    d = R.sparse_to_dense_fwd(X.numpy(), coords, grid, batch)
    assert np.array_equal(d, O.sparse_to_dense(X, coords, grid, batch).numpy())
    assert np.array_equal(R.sparse_to_dense_bwd(d, coords), X.numpy())
    Xn = -X.abs() - 1                                                     # all negative: amax must be negative
    for op, fn in (("mean", torch.mean), ("sum", torch.sum), ("amax", torch.amax)):
        y = R.segment_pool_fwd(Xn.numpy(), coords[:, 3], batch, op)
        yo = O.global_pool(Xn.double(), coords, batch, fn).numpy()
        np.testing.assert_allclose(y, yo, rtol=1e-14, atol=0)
        assert (y[1] == 0).all() and (y[[0, 2]] < 0).all()
        Xg = Xn.clone().requires_grad_()
        yg = O.global_pool(Xg, coords, batch, fn)
        gy = torch.randn(yg.shape, generator=torch.Generator().manual_seed(9))
        (ag,) = torch.autograd.grad(yg, Xg, gy)
        dx = R.segment_pool_bwd(Xn.numpy(), yg.detach().numpy(), gy.numpy(), coords[:, 3], batch, op)
        np.testing.assert_allclose(dx, ag.numpy(), rtol=2e-7, atol=0)
    # tied maxima share the gradient evenly (torch.amax), a -0 / +0 pair is a tie whose maximum is +0
    Xt = np.array([[1.0, -0.0], [1.0, 0.0], [0.5, -3.0]], dtype=np.float32)
    s = np.zeros(3, dtype=np.int64)
    y = R.segment_pool_fwd(Xt, s, 1, "amax")
    assert np.array_equal(y, [[1.0, 0.0]]) and not np.signbit(y).any()
    dx = R.segment_pool_bwd(Xt, y, np.array([[4.0, 6.0]], dtype=np.float32), s, 1, "amax")
    assert np.array_equal(dx, [[2.0, 3.0], [2.0, 3.0], [0.0, 0.0]])
    Xa = torch.from_numpy(Xt).requires_grad_()
    (ag,) = torch.autograd.grad(torch.amax(Xa, dim=0), Xa, torch.tensor([4.0, 6.0]))
    assert np.array_equal(ag.numpy(), dx)
