"""Pins tests/wgrad_restate.py (the numpy / float64 restatement the weight-gradient path tests compare against) on the CPU:
against torch.einsum / index_add_ in float64, the exactness precondition of the `exact` operand kind for every case of the
GPU file's tables, the rounding-error bound on fp32 accumulations in two orders -- and, without a GPU, that every row of the
shape table names the path scn_wgrad_plan_describe reports (the entry point is host-only)."""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_restate as R


def _torch_wgrad(X, dY, in_rows, out_rows, prefix, relu_in, db_mask):
    X, dY = torch.from_numpy(X).double(), torch.from_numpy(dY).double()
    if relu_in:
        X = X.clamp_min(0)
    n_off = len(prefix) - 1
    total = int(prefix[-1])
    if in_rows is None:
        in_rows = out_rows = np.arange(total)
    off = torch.from_numpy(np.repeat(np.arange(n_off), np.diff(prefix)))
    xi = X[torch.from_numpy(np.asarray(in_rows[int(prefix[0]):total])).long()]
    yo = dY[torch.from_numpy(np.asarray(out_rows[int(prefix[0]):total])).long()]
    terms = torch.einsum("pi,pj->pij", xi, yo)
    dW = torch.zeros(n_off, X.shape[1], dY.shape[1], dtype=torch.float64).index_add_(0, off, terms)
    S = torch.zeros_like(dW).index_add_(0, off, terms.abs())
    keep = torch.tensor([(db_mask >> o) & 1 for o in range(n_off)], dtype=torch.float64)[off]
    db = (yo * keep[:, None]).sum(0)
    return dW.numpy(), db.numpy(), S.numpy()


@pytest.mark.parametrize("counts,first,mask", [([0, 5, 0, 0, 17, 1], 0, 0b010010), ([9], 3, 1), ([4, 4, 0, 31], 0, 0b1111)])
@pytest.mark.parametrize("relu_in", [0, 1])
def test_restatement_equals_einsum_and_index_add(counts, first, mask, relu_in):
    in_rows, out_rows, prefix = R.rule_list(counts, n_in=11, n_out=7, seed=len(counts), first=first)
    assert int(prefix[0]) == first and len(in_rows) == first + sum(counts)
    X, dY = R.operand("gaussian", 11, 5, 1), R.operand("gaussian", 7, 3, 2)
    got = R.wgrad(X, dY, in_rows, out_rows, prefix, relu_in, mask)
    ref = _torch_wgrad(X, dY, in_rows, out_rows, prefix, relu_in, mask)
    for g, r in zip(got, ref):
        np.testing.assert_allclose(g, r, rtol=0, atol=1e-13)
    s_db, n_db = R.db_abs(dY, out_rows, prefix, mask)
    assert n_db == sum(c for o, c in enumerate(counts) if (mask >> o) & 1)
    np.testing.assert_allclose(s_db, np.abs(_torch_wgrad(X, np.abs(dY), in_rows, out_rows, prefix, 0, mask)[1]), rtol=0, atol=1e-13)


def test_identity_list_is_the_plain_product():
    X, dY = R.operand("exact", 13, 4, 3), R.operand("exact", 13, 6, 4)
    dW, db, S = R.wgrad(X, dY, None, None, [0, 13], 0, 1)
    assert np.array_equal(dW[0], X.astype(np.float64).T @ dY) and np.array_equal(db, dY.astype(np.float64).sum(0))
    assert np.array_equal(S[0], np.abs(X).astype(np.float64).T @ np.abs(dY))
    ref = _torch_wgrad(X, dY, None, None, np.array([0, 13]), 0, 1)
    assert np.array_equal(dW, ref[0])


def test_operand_kinds():
    x = R.operand("exact", 400, 50, 7)
    assert set(np.unique(x)) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    assert 0.30 < (x == 0).mean() < 0.37 and 0.30 < (x < 0).mean() < 0.37          # a third zeros, half of the rest negative
    g = R.operand("gaussian", 400, 50, 7, bf16=True)
    assert np.array_equal(g, torch.from_numpy(R.operand("gaussian", 400, 50, 7)).bfloat16().float().numpy())
    assert np.array_equal(R.from_bf16_bits(R.to_bf16_bits(x)), x)                       # small integers are bf16 numbers


def test_exactness_precondition_of_every_tabulated_case():
    """|x|, |dy| <= 3: S <= 9 N.  Checked on the lists themselves for the widest and the narrowest shape, and through the
    9 N bound for every shape x list (and for four problems: each problem is its own sum)."""
    for name in R.LISTS:
        in_rows, out_rows, prefix, mask = R.make_list(name)
        n_max = int(np.diff(prefix).max())
        assert 9 * n_max < R.EXACT_LIMIT and 3 * int(prefix[-1] - prefix[0]) < R.EXACT_LIMIT
        for cin, cout in [(256, 128), (1, 1)]:
            X, dY = R.operand("exact", R.N_IN, cin, 11), R.operand("exact", R.N_OUT, cout, 12)
            _, _, S = R.wgrad(X, dY, in_rows, out_rows, prefix, 0, mask)
            R.assert_exact(S, R.db_abs(dY, out_rows, prefix, mask)[0])
            assert S.max() <= 9 * n_max
    for n in R.IDENT_ROWS:
        assert 9 * n < R.EXACT_LIMIT
    for cin, cout, *_ in R.SHAPES:
        assert cin >= 1 and cout >= 1


def test_the_bound_holds_for_fp32_accumulation_in_two_orders():
    rng = np.random.default_rng(5)
    for n in (1, 4, 65, 1025):
        a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        exact = float(a.astype(np.float64) @ b.astype(np.float64))
        S = float(np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64))
        fwd = np.float32(0)
        for k in range(n):
            fwd = np.float32(fwd + np.float32(a[k] * b[k]))
        parts = [np.float32(a[k] * b[k]) for k in range(n)]                 # pairwise tree, from the far end
        parts.reverse()
        while len(parts) > 1:
            parts = [np.float32(parts[k] + parts[k + 1]) if k + 1 < len(parts) else parts[k] for k in range(0, len(parts), 2)]
        for got in (float(fwd), float(parts[0])):
            assert abs(got - exact) <= float(R.bound(n, S))
        assert float(R.bound(n, S)) < (n + 3) * R.U32 * S                     # (and it is no wider than it looks)


# ------------------------------------------------------------------------------------------------------------------------
# the path report (host only)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    from sparse_rcnn_amd import _lib
    return _lib


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_the_shape_table_names_the_reported_path(L, shape):
    cin, cout, bf16, sw, path = shape
    _, _, prefix, _ = R.make_list("A")
    lib = L.load()
    ph = (C.c_int64 * 28)(*[int(v) for v in prefix])
    for plan in R.PLANS:
        with R.switches(L, {**sw, **plan}):
            rc, d = R.describe(L, cin, cout, prefix, 1, bf16, 0, 0)
            assert rc == 0 and {k: d[k] for k in path} == path, (plan, d)
            counts = np.diff(prefix)
            assert d["units"] == int(np.sum(-(-counts // d["per"]))) and d["memset"] == 0
            if plan.get("SCN_WGRAD_SPLITS") == "4096":
                assert d["per"] == R.floor_per(path) and -(-1025 // d["per"]) == {512: 3, 128: 9, 256: 5}[d["per"]]
            if plan.get("SCN_WGRAD_SPLITS") == "1":
                assert d["units"] == int((counts > 0).sum())
            if plan.get("SCN_WGRAD_SPLITS") == "5":
                assert d["per"] > R.floor_per(path) and -(-1025 // d["per"]) == 2
            for n_prob in (1, 2, 4):
                rc, dn = R.describe(L, cin, cout, prefix, n_prob, bf16, 0, 0)
                size = lib.scn_wgrad_scratch_bytes(cin, cout, ph, 27) if n_prob == 1 else \
                    lib.scn_wgrad_scratch_bytes_n(cin, cout, ph, 27, n_prob)
                assert rc == 0 and 0 < dn["bytes"] < dn["bytes_db"] <= size - 512


def test_alignment_moves_the_reported_path_and_bad_arguments_are_refused(L):
    _, _, prefix, _ = R.make_list("A")
    _, d = R.describe(L, 64, 64, prefix, 1, False, 4, 0)
    assert (d["edge"], d["evec"], d["V"]) == (1, 0, 4)
    _, d = R.describe(L, 48, 48, prefix, 1, False, 4, 0)
    assert (d["ta"], d["edge"]) == (3, 0)
    _, d = R.describe(L, 64, 64, prefix, 1, True, 2, 0)
    assert (d["kernel"], d["hb"], d["edge"]) == ("d", 1, 1)
    _, d = R.describe(L, 64, 64, prefix, 1, False, 0, 4)
    assert (d["edge"], d["V"]) == (0, 1)
    _, d = R.describe(L, 64, 64, [0] * 28, 1, False, 0, 0)
    assert d["memset"] == 1 and d["units"] == 0 and d["bytes_db"] == 0
    assert R.describe(L, 64, 64, prefix, 1, False, 2, 0)[0] == L.EINVAL          # a float pointer two bytes off
    assert R.describe(L, 64, 64, prefix, 1, True, 1, 0)[0] == L.EINVAL
    assert R.describe(L, 64, 64, prefix, 5, False, 0, 0)[0] == L.EINVAL
    assert R.describe(L, 64, 64, [7] + list(prefix[1:]), 2, False, 0, 0)[0] == L.EINVAL      # several problems: prefix[0] = 0
    assert R.describe(L, 64, 64, [5, 3], 1, False, 0, 0)[0] == L.EINVAL
