"""Pins tests/conv_restate.py (the numpy / float64 restatement the tile-convolution path tests compare against) on the CPU:
against torch.nn.functional.conv3d and its autograd gradient in float64 (SubM 3^3 on a fully active grid, a stride-2 child
table), the mask / residual orders by hand, the exactness precondition of the `exact` operand kind for every tabulated case,
the rounding-error bound on fp32 accumulations in two orders -- and, without a GPU, that every row of the case table names the
path scn_conv_tiles_plan_describe reports (the entry point is host-only) and that the table reaches every branch of the
launcher."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_restate as R

GRID = (5, 6, 7)


def _subm_table(grid):
    """SubM 3^3 table of a fully active grid: table[o][r] = the row at r + (offset o - 1), -1 outside; rows and offsets in
    C order (x slowest), as conv3d orders its kernel."""
    gx, gy, gz = grid
    idx = np.arange(gx * gy * gz).reshape(grid)
    table = np.full((27, idx.size), -1, dtype=np.int32)
    for o, (dx, dy, dz) in enumerate(np.ndindex(3, 3, 3)):
        for x, y, z in np.ndindex(*grid):
            u, v, w = x + dx - 1, y + dy - 1, z + dz - 1
            if 0 <= u < gx and 0 <= v < gy and 0 <= w < gz:
                table[o][idx[x, y, z]] = idx[u, v, w]
    return table


def _child_table(grid):
    """2^3 stride-2 child table: table[o][coarse row] = the fine row at 2 * coarse + offset o (the grid's sizes are even)."""
    gx, gy, gz = grid
    idx = np.arange(gx * gy * gz).reshape(grid)
    coarse = np.arange(gx * gy * gz // 8).reshape(gx // 2, gy // 2, gz // 2)
    table = np.full((8, coarse.size), -1, dtype=np.int32)
    for o, (dx, dy, dz) in enumerate(np.ndindex(2, 2, 2)):
        for x, y, z in np.ndindex(*coarse.shape):
            table[o][coarse[x, y, z]] = idx[2 * x + dx, 2 * y + dy, 2 * z + dz]
    return table


def _dense(rows, grid):
    """[n, c] rows of a fully active grid -> [1, c, x, y, z]."""
    return torch.from_numpy(rows).double().reshape(*grid, -1).permute(3, 0, 1, 2)[None]


def _rows(dense):
    return dense[0].permute(1, 2, 3, 0).reshape(-1, dense.shape[1]).numpy()


def test_subm_forward_equals_conv3d_and_backward_data_its_input_gradient():
    cin, cout = 3, 4
    n = int(np.prod(GRID))
    table = _subm_table(GRID)
    X, W, b = R.operand("gaussian", n, cin, 1), R.operand("gaussian", 27 * cin, cout, 2).reshape(27, cin, cout), \
        R.operand("gaussian", 1, cout, 3)[0]
    Wt = torch.from_numpy(W).double().reshape(3, 3, 3, cin, cout).permute(4, 3, 0, 1, 2)          # [cout, cin, 3, 3, 3]
    xd = _dense(X, GRID).requires_grad_()
    yd = torch.nn.functional.conv3d(xd, Wt, torch.from_numpy(b).double(), padding=1)
    Y, S, N = R.conv(X, W, table, b, None, None, 0)
    np.testing.assert_allclose(Y, _rows(yd.detach()), rtol=0, atol=1e-13)
    assert np.array_equal(N, (table >= 0).sum(0) * cin + 1) and N.max() == 27 * cin + 1 and N.min() == 8 * cin + 1
    ref_S = _rows(torch.nn.functional.conv3d(xd.detach().abs(), Wt.abs(), torch.from_numpy(np.abs(b)).double(), padding=1))
    np.testing.assert_allclose(S, ref_S, rtol=0, atol=1e-13)
    # backward-data: dX = the SAME table walked with the transposed weights in reversed offset order
    dY = R.operand("gaussian", n, cout, 4)
    (gx,) = torch.autograd.grad(yd, xd, _dense(dY, GRID))
    dX, _, _ = R.conv(dY, W, table, None, None, None, R.F_W_TRANSPOSED | R.F_OFF_REVERSE)
    np.testing.assert_allclose(dX, _rows(gx), rtol=0, atol=1e-13)
    # the input ReLU
    Yr, _, _ = R.conv(X, W, table, b, None, None, R.F_RELU_IN)
    yr = torch.nn.functional.conv3d(xd.detach().clamp_min(0), Wt, torch.from_numpy(b).double(), padding=1)
    np.testing.assert_allclose(Yr, _rows(yr), rtol=0, atol=1e-13)
    # OFF_REVERSE alone: the kernel mirrored
    Ym, _, _ = R.conv(X, W, table, b, None, None, R.F_OFF_REVERSE)
    ym = torch.nn.functional.conv3d(xd.detach(), Wt.flip(2, 3, 4), torch.from_numpy(b).double(), padding=1)
    np.testing.assert_allclose(Ym, _rows(ym), rtol=0, atol=1e-13)


def test_child_table_forward_equals_stride2_conv3d_and_transposed_its_input_gradient():
    grid, cin, cout = (4, 6, 8), 5, 3
    coarse = tuple(g // 2 for g in grid)
    table = _child_table(grid)
    n, nc = int(np.prod(grid)), int(np.prod(coarse))
    X, W = R.operand("gaussian", n, cin, 5), R.operand("gaussian", 8 * cin, cout, 6).reshape(8, cin, cout)
    Wt = torch.from_numpy(W).double().reshape(2, 2, 2, cin, cout).permute(4, 3, 0, 1, 2)
    xd = _dense(X, grid).requires_grad_()
    yd = torch.nn.functional.conv3d(xd, Wt, None, stride=2)
    Y, _, N = R.conv(X, W, table, None, None, None, 0)
    np.testing.assert_allclose(Y, _rows(yd.detach()), rtol=0, atol=1e-13)
    assert np.all(N == 8 * cin) and Y.shape == (nc, cout)
    # the input gradient of the stride-2 convolution, stated as a scatter over the child table
    dY = R.operand("gaussian", nc, cout, 7)
    (gx,) = torch.autograd.grad(yd, xd, _dense(dY, coarse))
    gx = _rows(gx)
    want = np.zeros((n, cin))
    for o in range(8):
        want[table[o]] += dY.astype(np.float64) @ W[o].astype(np.float64).T
    np.testing.assert_allclose(gx, want, rtol=0, atol=1e-13)
    # W_TRANSPOSED alone: weights stored [o][cout][cin], used as [cin][cout]
    Yt, _, _ = R.conv(X, np.ascontiguousarray(W.transpose(0, 2, 1)), table, None, None, None, R.F_W_TRANSPOSED)
    np.testing.assert_allclose(Yt, Y, rtol=0, atol=1e-13)
    # Deconvolution backward-data has this form (a child table, W_TRANSPOSED alone).  Pinned against the gradient above: as a
    # gather, that gradient walks the table of each fine row's one parent with the transposed weights
    parent = np.full((8, n), -1, dtype=np.int32)
    for o in range(8):
        parent[o][table[o]] = np.arange(nc)
    dX, _, _ = R.conv(dY, W, parent, None, None, None, R.F_W_TRANSPOSED)
    np.testing.assert_allclose(dX, gx, rtol=0, atol=1e-13)


def test_mask_and_residual_orders_by_hand():
    X = np.array([[2.0]], dtype=np.float32)
    W = np.array([[[3.0, 3.0, 3.0, 3.0, 3.0]]], dtype=np.float32)               # 1 offset, 1 -> 5 channels: sum = 6
    table = np.array([[0]], dtype=np.int32)
    bias = np.full(5, 1.0, dtype=np.float32)
    res = np.full((1, 5), -10.0, dtype=np.float32)
    mask = np.array([[-2.0, -0.0, 0.0, 1.0, 3.0]], dtype=np.float32)
    Y, S, N = R.conv(X, W, table, bias, res, mask, 0)
    assert Y.tolist() == [[0.0, 0.0, 0.0, -3.0, -3.0]]                          # (1 + 6 - 10) where mask > 0
    assert S.tolist() == [[17.0] * 5] and N.tolist() == [3]
    Y, S, N = R.conv(X, W, table, bias, res, mask, R.F_RESIDUAL_LAST)
    assert Y.tolist() == [[-10.0, -10.0, -10.0, -3.0, -3.0]]                    # mask first, then the residual
    assert S.tolist() == [[17.0] * 5]
    Y, _, N = R.conv(X, W, table, None, None, np.array([[np.nan, 1, 1, 1, 1]], dtype=np.float32), 0)
    assert Y.tolist() == [[0.0, 6.0, 6.0, 6.0, 6.0]] and N.tolist() == [1]       # !(mask > 0): a NaN mask zeroes
    Y, _, N = R.conv(-X, W, table, bias, None, None, R.F_RELU_IN)
    assert Y.tolist() == [[1.0] * 5]
    Y, _, N = R.conv(X, W, np.array([[-1]], dtype=np.int32), bias, None, None, 0)
    assert Y.tolist() == [[1.0] * 5] and N.tolist() == [1]                       # a row without a rule: the bias alone
    assert set(np.unique(R.mask_operand(300, 7, 1)).tolist()) == {-2.0, 0.0, 1.0, 3.0}
    assert np.signbit(R.mask_operand(300, 7, 1)).sum() > (R.mask_operand(300, 7, 1) == -2).sum()          # -0.0 is drawn


def test_rule_tables_hold_their_recipe():
    for n_off in (27, 8, 12, 1):
        table, n_in = R.rule_table(n_off)
        n_out = table.shape[1]
        assert table.shape == (n_off, R.small_rows(n_off)) and n_out % 16 != 0 and n_in == R.N_IN_FACTOR[n_off] * n_out
        assert table.min() == -1 and table.max() == n_in - 1
        for o in (0, n_off - 1):
            assert 0 in table[o] and n_in - 1 in table[o]
        masks = ((table >= 0).astype(np.int64) << np.arange(n_off)[:, None]).sum(0)
        vals, counts = np.unique(masks, return_counts=True)
        pops = {bin(int(v)).count("1") for v, c in zip(vals, counts) if c >= R.GROUP_ROWS}
        assert set(R.group_counts(n_off)) <= pops
        if n_off == 27:
            assert np.all(table[13] >= 0)
        unnamed = R.unnamed_rows(table, n_in)
        assert len(unnamed) >= n_in // 5 - 2 and not np.isin(unnamed, table).any()
        # the numpy statement of the tile structures agrees with its own checker
        order = np.argsort(masks, kind="stable")
        nt = -(-n_out // 16)
        perm = np.concatenate([order, np.full(nt * 16 - n_out, -1)]).astype(np.int32)
        padded = np.concatenate([table, np.full((n_off, 1), -1, dtype=np.int32)], axis=1)
        tstab = np.ascontiguousarray(padded[:, perm].reshape(n_off, nt, 16).transpose(1, 0, 2))
        tmask = np.array([np.bitwise_or.reduce(np.where(perm[16 * t:16 * t + 16] >= 0, masks[perm[16 * t:16 * t + 16]], 0))
                          for t in range(nt)]).astype(np.uint32)
        pop = np.array([bin(int(m)).count("1") for m in tmask])
        pops_t = R.check_tiles(table, perm, tstab, tmask.view(np.int32), np.argsort(-pop, kind="stable").astype(np.int32))
        assert set(R.group_counts(n_off)) <= set(pops_t.tolist())
    long_table, _ = R.rule_table(27, 16 * 64 * 2 + 5)
    assert long_table.shape == (27, 2053)


def test_exactness_precondition_of_every_tabulated_case():
    """|x|, |w| <= 3: a row's S <= 9 * cin * (its rules) + |bias| + |residual| <= 27 * 160 * 9 + 6.  Through that bound for every
    case, and on the operands themselves for the widest and the narrowest shape."""
    for c in R.CASES:
        assert c.cin <= 160 and c.n_off <= 27
        assert 9 * c.cin * c.n_off + 6 < R.EXACT_LIMIT
    assert 27 * 160 * 9 + 6 < R.EXACT_LIMIT
    table, n_in = R.rule_table(27)
    for cin, cout in ((160, 32), (3, 5)):
        X, W = R.operand("exact", n_in, cin, 11), R.operand("exact", 27 * cin, cout, 12).reshape(27, cin, cout)
        b, r = R.operand("exact", 1, cout, 13)[0], R.operand("exact", table.shape[1], cout, 14)
        Y, S, N = R.conv(X, W, table, b, r, R.mask_operand(table.shape[1], cout, 15), R.F_RESIDUAL_LAST)
        R.assert_exact(S)
        assert S.max() <= 9 * cin * 27 + 6 and np.array_equal(Y, np.round(Y)) and N.max() == 27 * cin + 2


def test_the_bound_holds_for_fp32_accumulation_in_two_orders():
    """A whole row of the restatement: N = cin * rules + 2 terms, summed in fp32 front to back and as a pairwise tree from the
    far end (bias and residual among the terms)."""
    table, n_in = R.rule_table(27)
    cin, cout = 32, 4
    X, W = R.operand("gaussian", n_in, cin, 21), R.operand("gaussian", 27 * cin, cout, 22).reshape(27, cin, cout)
    b, r = R.operand("gaussian", 1, cout, 23)[0], R.operand("gaussian", table.shape[1], cout, 24)
    Y, S, N = R.conv(X, W, table, b, r, None, 0)
    for row in (0, 17, 400, table.shape[1] - 1):
        for n in range(cout):
            terms = [b[n]] + [np.float32(X[table[o][row]][k] * W[o][k][n]) for o in range(27) if table[o][row] >= 0
                              for k in range(cin)] + [r[row][n]]
            assert len(terms) == N[row]
            fwd = np.float32(0)
            for t in terms:
                fwd = np.float32(fwd + t)
            parts = list(reversed(terms))
            while len(parts) > 1:
                parts = [np.float32(parts[k] + parts[k + 1]) if k + 1 < len(parts) else parts[k] for k in range(0, len(parts), 2)]
            lim = float(R.bound(N[row], S[row][n]))
            for got in (float(fwd), float(parts[0])):
                assert abs(got - Y[row][n]) <= lim
            assert lim < (N[row] + 3) * R.U32 * S[row][n]


# ------------------------------------------------------------------------------------------------------------------------
# the path report (host only)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import __graft_entry__
    __graft_entry__.build()
    from sparse_rcnn_amd import _lib
    return _lib


def _report(L, c):
    rows = R.table_rows(L, c)
    n_in = R.N_IN_FACTOR[c.n_off] * rows
    with R.switches(L, c.sw):
        rc, d = R.describe(L, n_in, c.cin, c.n_off, rows, c.cout, c.flags, c.arrival, *c.ptr_bits())
    assert rc == 0
    return rows, d


@pytest.mark.parametrize("group", R.GROUPS)
def test_every_case_names_the_reported_path(L, group):
    lib = L.load()
    for c in [c for c in R.CASES if c.group == group]:
        rows, d = _report(L, c)
        assert {k: d[k] for k in c.expect} == c.expect, (c.id(), d)
        nt = -(-rows // 16)
        assert 1 <= d["n_tg"] <= -(-nt // (4 if d["split4"] else 16)) and d["grid_x"] >= d["n_kc"] * d["n_chunks"]
        if not d["tail"]:
            assert d["grid_x"] == d["n_tg"] * d["n_kc"] * d["n_chunks"]
        if c.table == "long":                                        # the plain loop: ~4 tiles per wave of the busiest slice
            assert not d["split4"] and 3.5 <= nt / (16 * d["n_tg"]) <= 4.5, (c.id(), d)
        if c.table == "long4":                                       # the four-wave loop: at least three rounds
            assert d["split4"] and -(-(nt // d["n_tg"]) // 4) >= 3, (c.id(), d)
        if c.table == "small" and d["split4"] and not c.sw.get("SCN_CU_BUDGET"):
            assert -(-nt // d["n_tg"]) <= 4                          # one round
        assert lib.scn_conv_tiles_arrival_counters(c.cin, rows, c.cout) == (nt * d["n_chunks"] if d["n_kc"] > 1 else 0)
        assert lib.scn_conv_tiles_scratch_bytes(c.cin, rows, c.cout) == \
            256 + (d["n_kc"] * nt * 16 * d["n_chunks"] * 32 * 4 if d["n_kc"] > 1 else 0)


def test_the_case_table_reaches_every_branch_of_the_launcher(L):
    """The (FULLK, staging, PART, TAIL, FUSED, SPLIT) tuples scn_conv_tiles_plan_describe reports over the table are exactly
    the k_conv_ts instantiations the launcher can choose for cin <= 160; the stream kernel is reported where it is asked for."""
    reached, streams = set(), 0
    for c in R.CASES:
        _, d = _report(L, c)
        b = R.branch_of(d)
        if b is None:
            streams += 1
        else:
            reached.add(b)
    assert reached == R.LAUNCH_BRANCHES, (R.LAUNCH_BRANCHES - reached, reached - R.LAUNCH_BRANCHES)
    assert streams == sum(c.expect["stream"] for c in R.CASES) == 12
    # and what the table names beyond the instantiation: both K-chunk sums, the combiner's second pass, every PROG depth, the
    # both-only slice class, K tails of 4 / 8 / 12 / 16 channels
    assert {(c.expect["finish_v4"]) for c in R.CASES if c.expect["n_kc"] > 1 and not c.expect["fused"]} == {0, 1}
    assert any(c.expect["n_kc"] > 4 and c.expect["fused"] for c in R.CASES)
    assert {c.expect["prog_g0"] for c in R.CASES} == {0, 4, 8, 12}
    assert {c.cin % 32 for c in R.CASES if c.expect["tail"] and c.expect["k_tail"]} >= {4, 8, 12, 16}
    assert any(c.expect["tail"] and c.expect["n_kc"] == 1 and c.expect["n_chunks"] == 1 and c.expect["k_tail"]
               and c.expect["n_tail"] for c in R.CASES)
    assert sum(c.gaussian for c in R.CASES) >= len(R.LAUNCH_BRANCHES)


def test_switches_and_alignment_move_the_reported_path(L):
    def d(cin, cout, flags=0, arrival=True, n=889, n_off=27, **bits):
        rc, out = R.describe(L, n, cin, n_off, n, cout, flags, arrival, **bits)
        assert rc == 0
        return out

    base = d(64, 64)
    assert (base["fullk"], base["vecn"], base["fused"], base["split4"], base["finish_v4"]) == (1, 1, 1, 1, 1)
    assert d(64, 64, x_bits=4)["fullk"] == 0 and d(64, 64, x_bits=4)["vecn"] == 1
    assert d(64, 64, w_bits=8)["fullk"] == 0 and d(64, 64, w_bits=8)["vecn"] == 0
    assert d(64, 64, epi_bits=4)["finish_v4"] == 0 and d(64, 64, epi_bits=4)["fullk"] == 1
    assert d(64, 64, arrival=False)["fused"] == 0 and d(64, 64, R.F_SPLIT_SUM)["fused"] == 0
    assert d(64, 64, n=40000)["split4"] == 0                         # 2500 tiles x 4 slices > 2048
    assert d(32, 32, n=16 * 2048)["split4"] == 1 and d(32, 32, n=16 * 2048 + 1)["split4"] == 0
    with L.debug_switch("SCN_TS_SPLIT", 0):
        assert d(64, 64)["split4"] == 0
        with L.debug_switch("SCN_TS_PROG", 7):
            assert d(64, 64)["prog_g0"] == 8 and d(64, 64, R.F_W_TRANSPOSED)["prog_g0"] == 0 and d(64, 64, n_off=8)["prog_g0"] == 0
        with L.debug_switch("SCN_TS_PROG", 13):
            assert d(64, 64)["prog_g0"] == 0
    with L.debug_switch("SCN_TS_NO_TAIL", 1):
        t = d(48, 48)
        assert (t["tail"], t["k_tail"], t["n_tail"]) == (0, 1, 1) and t["grid_x"] == t["n_tg"] * 4
    t = d(48, 48)
    assert t["tail"] == 1 and t["grid_x"] > t["n_tg"] * 2            # four slice classes with their own shares
    with L.debug_switch("SCN_TS_STREAM", 1):
        assert d(64, 64)["stream"] == 1 and d(64, 64, R.F_SPLIT_SUM)["stream"] == 0 and d(64, 64, arrival=False)["stream"] == 0
        assert d(64, 64, x_bits=4)["stream"] == 0 and d(96, 64)["stream"] == 0 and d(64, 32)["stream"] == 0
        assert d(64, 64, n_off=12)["stream"] == 0 and d(128, 64, n_off=8)["stream"] == 1
    assert d(64, 64)["stream"] == 0
    with L.debug_switch("SCN_CU_BUDGET", 32):
        assert d(32, 32, n=40000)["n_tg"] == 32 and d(64, 64, n=40000)["n_tg"] == 8 and d(128, 128, n=40000)["n_tg"] == 2
    assert d(32, 32, n=40000)["n_tg"] == cdiv(cdiv(40000, 16), 16)
    zero = d(64, 64, n=0)
    assert all(v == 0 for v in zero.values())


def cdiv(a, b):
    return -(-a // b)


def test_bad_arguments_and_half_aligned_pointer_bits_are_refused(L):
    lib = L.load()
    out = (C.c_int64 * 16)()
    ok = (889, 32, 27, 889, 32, 0, 1, 0, 0)
    assert lib.scn_conv_tiles_plan_describe(*ok, out) == L.OK
    for pos, bad in ((2, 28), (2, 0), (1, 0), (4, 0), (0, -1), (3, -1), (7, 2), (7, 1), (7, 6), (8, 2), (8, 1), (8, 16), (7, 256),
                     (7, 0x40), (7, 0x84)):                           # (W's bits are a subset of X | W's)
        args = list(ok)
        args[pos] = bad
        assert lib.scn_conv_tiles_plan_describe(*args, out) == L.EINVAL, (pos, bad)
    assert lib.scn_conv_tiles_plan_describe(*ok, None) == L.EINVAL
    for good in ((7, 4), (7, 0x44), (7, 0xCC), (7, 0x4C), (8, 4), (8, 12)):
        args = list(ok)
        args[good[0]] = good[1]
        assert lib.scn_conv_tiles_plan_describe(*args, out) == L.OK, good
